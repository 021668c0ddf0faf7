// orb_hamming.h -- the 256-bit Hamming distance of two ORB descriptors (ORBmatcher::DescriptorDistance, src/ORBmatcher.cc:2058-2074)
// as the search kernels of orb_device.hip, stereo_device.hip and fisheye_stereo_device.hip compute it, and the packing of their keys.
#pragma once
#include <hip/hip_runtime.h>

namespace osh {

// The search kernels keep a candidate as the key (distance << kPosBits) | index and take the minimum: a Hamming distance is at
// most 256 (9 bits), an index is below 2^22, and the all-ones key means none.  The entries refuse a larger train set.
constexpr int kPosBits = 22;
constexpr unsigned kPosMask = (1u << kPosBits) - 1;

// popcount(x) + acc in ONE instruction (v_bcnt_u32_b32 adds its second operand).  Written as `__builtin_popcount(x) + acc` the
// compiler re-associates the eight terms of a distance into separate counts and a tree of v_add3_u32: 3 extra lane-ops per pair
// (22.8 measured against the 16 of eight xor + eight chained counts).
__device__ __forceinline__ unsigned bcnt_acc(unsigned x, unsigned acc) {
  unsigned r;
  asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(acc));
  return r;
}
__device__ __forceinline__ unsigned hamming256(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
  unsigned d = __builtin_popcount(a0.x ^ b0.x);
  d = bcnt_acc(a0.y ^ b0.y, d);
  d = bcnt_acc(a0.z ^ b0.z, d);
  d = bcnt_acc(a0.w ^ b0.w, d);
  d = bcnt_acc(a1.x ^ b1.x, d);
  d = bcnt_acc(a1.y ^ b1.y, d);
  d = bcnt_acc(a1.z ^ b1.z, d);
  d = bcnt_acc(a1.w ^ b1.w, d);
  return d;
}

}  // namespace osh
