// common.h -- error plumbing shared by the HIP translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <initializer_list>
#include "../../include/orbslam3_hip.h"

namespace osh {

// thread-local text returned by osh_last_error()
void set_error(const char* fmt, ...);
const char* get_error();

#define OSH_HIP(call)                                                                      \
  do {                                                                                     \
    hipError_t _e = (call);                                                                \
    if (_e != hipSuccess) {                                                                \
      osh::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(_e)); \
      return OSH_ERR_DEVICE;                                                               \
    }                                                                                      \
  } while (0)

#define OSH_TRY(expr) do { int _rc = (expr); if (_rc != OSH_OK) return _rc; } while (0)

// The solvers that run on an osh_lba_ctx besides the visual BA (pose_device.hip, posei_device.hip, sim3opt_device.hip,
// liba_device.hip and the pose graphs of pgo_env.h) share its device and stream, and keep their staging and work buffers in its
// attachment slots (a StagedCall each, PgoBuffers for the pose graphs; defined in lba_device.hip, the driver of the kernels in lba_*.h).
enum LbaAttachSlot { kAttachLiba = 0, kAttachPose = 1, kAttachPosei = 2, kAttachPgo = 3, kAttachSim3 = 4, kAttachCount };
// The context's device (made current) and stream.
int lba_stream(osh_lba_ctx* c, int* device, hipStream_t* stream);
// The context's pointer for `slot` (null until the caller stores its state there); osh_lba_destroy hands it to free_fn.
void** lba_attachment(osh_lba_ctx* c, LbaAttachSlot slot, void (*free_fn)(void*));
// The T kept in `slot`, created on first use and deleted by osh_lba_destroy (null without a context).
template <class T>
T* attachment(osh_lba_ctx* c, LbaAttachSlot slot) {
  void** p = lba_attachment(c, slot, [](void* q) { delete static_cast<T*>(q); });
  if (!p) { set_error("no context"); return nullptr; }
  if (!*p) *p = new T();
  return static_cast<T*>(*p);
}

// osh_orb_stereo_match (stereo_device.hip), osh_orb_fisheye_stereo_match (fisheye_stereo_device.hip) and osh_orb_bow_transform
// (bow_device.hip), osh_orb_bow_db_query (bowdb_device.hip), osh_orb_triangulate_new_points (newpoint_device.hip) and
// osh_orb_fast_detect / osh_orb_ic_angle (orb_fast_device.hip), osh_orb_describe (orb_brief_device.hip), osh_orb_refresh_map_points
// (mappoint_device.hip), osh_orb_two_view_reconstruct (two_view_device.hip), osh_orb_mlpnp_solve (mlpnp_device.hip), osh_orb_sim3_ransac (sim3_ransac_device.hip), osh_orb_octree_distribute (orb_octree_device.hip), osh_orb_extract (orb_extract_device.hip), osh_orb_keyframe_cull_stage / _count (keyframe_cull_device.hip), osh_orb_prepare / osh_orb_extract_raw (orb_prepare_device.hip), osh_orb_fuse_search (orb_fuse_device.hip) run on an osh_orb_ctx the same way: the context's device (made current) and stream, one attachment pointer each (handed to free_fn by osh_orb_destroy;
// orb_state of orb_stage.h is the typed fetch-or-create), and whether osh_orb_set_profiling switched timing on.
enum OrbAttachSlot { kOrbAttachStereo = 0, kOrbAttachFisheye = 1, kOrbAttachBow = 2, kOrbAttachBowDb = 3, kOrbAttachNewPoint = 4, kOrbAttachFast = 5, kOrbAttachBrief = 6, kOrbAttachMapPoint = 7, kOrbAttachTwoView = 8, kOrbAttachMlpnp = 9, kOrbAttachSim3Ransac = 10, kOrbAttachOctree = 11, kOrbAttachExtract = 12, kOrbAttachKfCull = 13, kOrbAttachPrepare = 14, kOrbAttachFuse = 15, kOrbAttachCount };
int orb_stream(osh_orb_ctx* c, int* device, hipStream_t* stream);
void** orb_attachment(osh_orb_ctx* c, void (*free_fn)(void*), OrbAttachSlot slot);
bool orb_profiling(osh_orb_ctx* c);

// OSH_ERR_DEVICE (with `what` in the message) if the last kernel launch failed.
int launch_check(const char* what);
// Opts each kernel in to `bytes` of dynamic LDS on `device`, the current device; the attribute is per kernel and device, so it is set
// once per pair in the process.
int allow_dynamic_lds(int device, int bytes, std::initializer_list<const void*> kernels);
template <class... K>
int allow_dynamic_lds(int device, int bytes, K... kernels) { return allow_dynamic_lds(device, bytes, {(const void*)kernels...}); }

// OSH_ZERO_NEW_BUFFERS=1 (a test aid, read at every allocation): every new device or pinned allocation of a context is zero-filled
// before it is handed out, so that what a call reads without having written it no longer depends on which memory the allocator
// recycled.  Zero only: it is a valid index and a harmless double everywhere.
inline bool zero_new_buffers() {
  const char* e = std::getenv("OSH_ZERO_NEW_BUFFERS");
  return e && std::strcmp(e, "1") == 0;
}
// Zero-fills `bytes` of device memory at `p` when OSH_ZERO_NEW_BUFFERS=1, complete on return (the contexts' streams do not wait for
// the null stream).
inline int zero_new_device(void* p, size_t bytes) {
  if (!zero_new_buffers()) return OSH_OK;
  OSH_HIP(hipMemset(p, 0, bytes));
  OSH_HIP(hipStreamSynchronize(nullptr));
  return OSH_OK;
}
inline void zero_new_host(void* p, size_t bytes) {
  if (zero_new_buffers()) std::memset(p, 0, bytes);
}

// Simple growable device buffer (never shrinks; reused across batches).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }   // owners that live in thread_local storage give their memory back when the thread exits
  int reserve(size_t bytes) {
    if (bytes <= cap) return OSH_OK;
    if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
    size_t want = bytes + bytes / 8 + 256;
    OSH_HIP(hipMalloc(&p, want));
    cap = want;
    return zero_new_device(p, want);
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; cap = 0; } }
  template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Pinned host buffer (grow-only).
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  void* reserve(size_t bytes) {
    if (bytes <= cap) return p;
    release();
    const size_t want = bytes + bytes / 8 + 4096;   // slack, as DevBuf: pinning is slow, a slightly larger batch reuses the buffer
    if (hipHostMalloc(&p, want) != hipSuccess) { p = nullptr; cap = 0; return nullptr; }
    cap = want;
    zero_new_host(p, want);
    return p;
  }
  void release() { if (p) { (void)hipHostFree(p); p = nullptr; cap = 0; } }
};

// One section of a Layout: an offset, turned into a typed pointer in a given base (host staging or device arena).
template <class T>
struct Section {
  size_t off;
  T* in(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
  const T* in(const void* base) const { return reinterpret_cast<const T*>(static_cast<const char*>(base) + off); }
};
// Sections laid out one after another, each 256-byte aligned and at least 8 bytes long (an empty one still has an address of its own).
struct Layout {
  size_t bytes = 0;
  template <class T>
  Section<T> take(size_t count) {
    const Section<T> s{bytes};
    bytes = (bytes + std::max<size_t>(count * sizeof(T), 8) + 255) & ~(size_t)255;
    return s;
  }
};

// The buffers of a one-launch solver call: the inputs staged in one pinned buffer and uploaded in one copy, the results downloaded in
// one copy into another (a copy per array cost more than a single frame's solve).  The device arena is [in | out | work].
struct StagedCall {
  PinBuf h_in, h_out;
  DevBuf arena;
  size_t in_bytes = 0, out_bytes = 0;
  int reserve(const Layout& in, const Layout& out, size_t work_bytes = 0, size_t min_arena_bytes = 0);
  char* host_in() const { return static_cast<char*>(h_in.p); }
  char* host_out() const { return static_cast<char*>(h_out.p); }
  char* dev_in() const { return arena.as<char>(); }
  char* dev_out() const { return dev_in() + in_bytes; }
  char* dev_work() const { return dev_out() + out_bytes; }
  int upload(hipStream_t s);     // h_in -> [in]
  int download(hipStream_t s);   // [out] -> h_out, then the stream synchronised
};

// Per-kernel HIP-event timing on one stream.
struct KernelTimer {
  static constexpr int kMaxPending = 4096;
  hipEvent_t ev[kMaxPending][2];
  int kid[kMaxPending];
  int n_pending = 0;
  bool created = false;
  bool enabled = false;
  int64_t launches[16] = {0};
  double total_ms[16] = {0};
  int init() {
    if (created) return OSH_OK;
    for (int i = 0; i < kMaxPending; ++i) {
      OSH_HIP(hipEventCreate(&ev[i][0]));
      OSH_HIP(hipEventCreate(&ev[i][1]));
    }
    created = true;
    return OSH_OK;
  }
  void destroy() {
    if (!created) return;
    for (int i = 0; i < kMaxPending; ++i) { (void)hipEventDestroy(ev[i][0]); (void)hipEventDestroy(ev[i][1]); }
    created = false;
  }
  void reset() { for (int i = 0; i < 16; ++i) { launches[i] = 0; total_ms[i] = 0; } n_pending = 0; }
  inline bool begin(int k, hipStream_t s) {
    if (!enabled || n_pending >= kMaxPending) return false;
    kid[n_pending] = k;
    (void)hipEventRecord(ev[n_pending][0], s);
    return true;
  }
  inline void end(hipStream_t s) { (void)hipEventRecord(ev[n_pending][1], s); ++n_pending; }
  // call after the stream has been synchronised
  void collect() {
    for (int i = 0; i < n_pending; ++i) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev[i][0], ev[i][1]) == hipSuccess) { launches[kid[i]]++; total_ms[kid[i]] += ms; }
    }
    n_pending = 0;
  }
};

}  // namespace osh
