// Micro-benchmark (not product code): can v_mfma_f64_4x4x4_4b_f64 (four independent 4x4x4 blocks per instruction) stand in for
// v_mfma_f64_16x16x4_f64 on the diagonal and ragged tiles of k_schur_fused?  Three questions:
//   1. lane layout of the operands and the result (block, row, k per lane; what cbsz / abid broadcast)
//   2. cycles per instruction: a dependent chain, an independent stream, and beside FP64 VALU work
//   3. bits: 24 k steps accumulated with 16x16x4 against the same entries accumulated with 4x4x4 blocks in the same k order
//   hipcc --offload-arch=gfx950 -O3 -o mfma_f64_blocks mfma_f64_blocks.hip && ./mfma_f64_blocks
// Exit status 0: all three answered and (3) identical; 2: layout not found; 3: bits differ.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

// ---------------------------------------------------------------------------------------- 1. layout
// One-hot probe: for every A lane la, a = [lane == la], b = 1 + lane: out[la][lane] = 1 + (the B lane that met A lane la in
// result lane `lane`), or 0 where A lane la does not reach that result lane.
template <int CBSZ, int ABID>
__global__ __launch_bounds__(64) void k_probe(double* out) {
  const int lane = threadIdx.x;
  for (int la = 0; la < 64; ++la) {
    const double a = lane == la ? 1.0 : 0.0, b = 1.0 + lane;
    out[la * 64 + lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, CBSZ, ABID, 0);
  }
}
// index-coded operands (small integers: every product and sum is exact) for the comparison with a triple loop on the host
__global__ __launch_bounds__(64) void k_coded(const double* a, const double* b, const double* c, double* d) {
  const int lane = threadIdx.x;
  d[lane] = __builtin_amdgcn_mfma_f64_4x4x4f64(a[lane], b[lane], c[lane], 0, 0, 0);
}

// A lane layout as three 2-bit fields of the lane number: shift of the block, the row (column for B / D's second index) and k fields
struct Fields { int blk, idx, k; };
static const int kPerm[6][3] = {{0, 2, 4}, {0, 4, 2}, {2, 0, 4}, {2, 4, 0}, {4, 0, 2}, {4, 2, 0}};
__host__ __device__ static inline int fld(int lane, int sh) { return (lane >> sh) & 3; }

// ---------------------------------------------------------------------------------------- 2. cycles
// Per iteration every mode issues the same matrix flop: 4 x 16x16x4 or 16 x (four blocks of 4x4x4); VALU modes 64 v_fma_f64.
//   0: 16x16x4, one dependent chain      1: 16x16x4, four independent accumulators
//   2: 4x4x4 blocks, one dependent chain 3: 4x4x4 blocks, sixteen independent accumulators
//   4: VALU only                         5: mode 1 + VALU interleaved   6: mode 3 + VALU interleaved
// (launch bounds of 512 as in f64_overlap.hip: with 64 the compiler copies every accumulator through AGPRs once per iteration)
template <int MODE>
__global__ __launch_bounds__(512) void k_time(double* out, long long* cyc, int iters, double seed) {
  f64x4 acc[4];
  double blk[16], v[16];
  for (int i = 0; i < 4; ++i) acc[i] = (f64x4){seed, seed, seed, seed};
  for (int i = 0; i < 16; ++i) { blk[i] = seed; v[i] = seed + i; }
  const double a = seed + threadIdx.x, b = seed * 0.5;
  constexpr bool valu = MODE >= 4;
  const long long t0 = clock64();
  for (int it = 0; it < iters; ++it) {
    if (MODE == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[0], 0, 0, 0);
    } else if (MODE == 1 || MODE == 5) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        acc[r] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[r], 0, 0, 0);
        if (valu) {
#pragma unroll
          for (int i = 0; i < 16; ++i) v[i] = __builtin_fma(v[i], 1.0000001, 0.5);
        }
      }
    } else if (MODE == 2) {
#pragma unroll
      for (int r = 0; r < 16; ++r) blk[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, blk[0], 0, 0, 0);
    } else if (MODE == 3 || MODE == 6) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        blk[r] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, blk[r], 0, 0, 0);
        if (valu) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[4 * (r & 3) + i] = __builtin_fma(v[4 * (r & 3) + i], 1.0000001, 0.5);
        }
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = __builtin_fma(v[i], 1.0000001, 0.5);
    }
  }
  const long long t1 = clock64();
  double s = 0;
  for (int i = 0; i < 4; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
  for (int i = 0; i < 16; ++i) s += blk[i] + v[i];
  out[blockIdx.x * 256 + threadIdx.x] = s;
  if (threadIdx.x == 0) cyc[blockIdx.x] = t1 - t0;
}

// one wavefront per SIMD: on one CU (clock64 ticks of wavefront 0), then on every CU (256 blocks, event time)
template <int MODE>
static int time_mode(const char* name, int per_iter, double* out, long long* cyc, double* cycles_one) {
  const int iters = 100000;
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  hipLaunchKernelGGL(k_time<MODE>, dim3(1), dim3(256), 0, 0, out, cyc, 100, 1.0);
  hipLaunchKernelGGL(k_time<MODE>, dim3(1), dim3(256), 0, 0, out, cyc, iters, 1.0);
  CHECK(hipDeviceSynchronize());
  long long c1 = 0;
  CHECK(hipMemcpy(&c1, cyc, sizeof c1, hipMemcpyDeviceToHost));
  CHECK(hipEventRecord(e0));
  hipLaunchKernelGGL(k_time<MODE>, dim3(256), dim3(256), 0, 0, out, cyc, iters, 1.0);
  CHECK(hipEventRecord(e1));
  CHECK(hipEventSynchronize(e1));
  float ms = 0;
  CHECK(hipEventElapsedTime(&ms, e0, e1));
  *cycles_one = (double)c1 / iters;
  printf("  %-46s one CU: %8.1f clock ticks / iteration", name, *cycles_one);
  if (per_iter) printf(" = %6.2f / instruction", *cycles_one / per_iter);
  printf("   256 CUs: %.3f ms\n", ms);
  return 0;
}

// ---------------------------------------------------------------------------------------- 3. bits
constexpr int kRows = 16, kK = 96;   // 24 k steps of 4 columns, four chunks of 8 landmarks
// D = WA WB^T with 16x16x4: lane holds A[row = lane & 15][k = lane >> 4], D[row = (lane >> 4) + 4 reg][col = lane & 15]
__global__ __launch_bounds__(64) void k_bits_tile(const double* wa, const double* wb, double* out, int ksteps) {
  const int lane = threadIdx.x, mrow = lane & 15, mk = lane >> 4;
  const double* A = wa + (size_t)blockIdx.x * kRows * kK;
  const double* B = wb + (size_t)blockIdx.x * kRows * kK;
  f64x4 acc = (f64x4){0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < ksteps; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A[mrow * kK + 4 * ks + mk], B[mrow * kK + 4 * ks + mk], acc, 0, 0, 0);
  for (int reg = 0; reg < 4; ++reg) out[(size_t)blockIdx.x * 256 + ((lane >> 4) + 4 * reg) * 16 + (lane & 15)] = acc[reg];
}
// the same 256 entries as 16 blocks of 4x4, four to an instruction: block pair p = 4 q + block, rows 4 (p >> 2) .., columns 4 (p & 3) ..
__global__ __launch_bounds__(64) void k_bits_blocks(const double* wa, const double* wb, double* out, int ksteps, Fields fa, Fields fb, Fields fd) {
  const int lane = threadIdx.x;
  const double* A = wa + (size_t)blockIdx.x * kRows * kK;
  const double* B = wb + (size_t)blockIdx.x * kRows * kK;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < ksteps; ++ks) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int pa = 4 * q + fld(lane, fa.blk), pb = 4 * q + fld(lane, fb.blk);
      const double a = A[(4 * (pa >> 2) + fld(lane, fa.idx)) * kK + 4 * ks + fld(lane, fa.k)];
      const double b = B[(4 * (pb & 3) + fld(lane, fb.idx)) * kK + 4 * ks + fld(lane, fb.k)];
      acc[q] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, acc[q], 0, 0, 0);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = 4 * q + fld(lane, fd.blk);
    out[(size_t)blockIdx.x * 256 + (4 * (p >> 2) + fld(lane, fd.idx)) * 16 + 4 * (p & 3) + fld(lane, fd.k)] = acc[q];
  }
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static double urand() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return (double)(g_rng >> 11) / 9007199254740992.0; }

template <int CBSZ, int ABID>
static int probe_broadcast(double* dout, const Fields& fa, const Fields& fd) {
  std::vector<double> h(64 * 64);
  hipLaunchKernelGGL((k_probe<CBSZ, ABID>), dim3(1), dim3(64), 0, 0, dout);
  CHECK(hipMemcpy(h.data(), dout, h.size() * sizeof(double), hipMemcpyDeviceToHost));
  int src[4] = {-1, -1, -1, -1};   // A block that reaches result block b (-2: more than one)
  for (int la = 0; la < 64; ++la)
    for (int lo = 0; lo < 64; ++lo)
      if (h[la * 64 + lo] != 0.0) {
        int& s = src[fld(lo, fd.blk)];
        const int ab = fld(la, fa.blk);
        s = (s == -1 || s == ab) ? ab : -2;
      }
  printf("  cbsz=%d abid=%d: result blocks 0..3 take their A operand from A blocks %d %d %d %d\n", CBSZ, ABID, src[0], src[1], src[2], src[3]);
  return 0;
}

int main() {
  double *dout, *da, *db, *dc;
  long long* dcyc;
  CHECK(hipMalloc(&dout, 256 * 256 * sizeof(double)));
  CHECK(hipMalloc(&da, 64 * sizeof(double))); CHECK(hipMalloc(&db, 64 * sizeof(double))); CHECK(hipMalloc(&dc, 64 * sizeof(double)));
  CHECK(hipMalloc(&dcyc, 1024 * sizeof(long long)));

  // ---- 1. layout
  printf("1. lane layout of v_mfma_f64_4x4x4_4b_f64\n");
  std::vector<double> hp(64 * 64);
  hipLaunchKernelGGL((k_probe<0, 0>), dim3(1), dim3(64), 0, 0, dout);
  CHECK(hipMemcpy(hp.data(), dout, hp.size() * sizeof(double), hipMemcpyDeviceToHost));
  printf("  one-hot probe, A lane -> (result lane : B lane) ...\n");
  for (int la = 0; la < 64; ++la) {
    if (!(la < 8 || la == 16 || la == 32 || la == 63)) continue;
    printf("   A lane %2d:", la);
    for (int lo = 0; lo < 64; ++lo) if (hp[la * 64 + lo] != 0.0) printf(" (%d : %d)", lo, (int)hp[la * 64 + lo] - 1);
    printf("\n");
  }
  double ha[64], hb[64], hc[64], hd[64];
  for (int i = 0; i < 64; ++i) { ha[i] = 1 + (i * 7) % 61; hb[i] = 2 + (i * 11) % 59; hc[i] = 1000 * i; }
  CHECK(hipMemcpy(da, ha, sizeof ha, hipMemcpyHostToDevice)); CHECK(hipMemcpy(db, hb, sizeof hb, hipMemcpyHostToDevice)); CHECK(hipMemcpy(dc, hc, sizeof hc, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_coded, dim3(1), dim3(64), 0, 0, da, db, dc, dout);
  CHECK(hipMemcpy(hd, dout, sizeof hd, hipMemcpyDeviceToHost));
  Fields fa{}, fb{}, fd{};
  int found = 0;
  for (int pa = 0; pa < 6; ++pa)
    for (int pb = 0; pb < 6; ++pb)
      for (int pd = 0; pd < 6; ++pd) {
        const Fields A{kPerm[pa][0], kPerm[pa][1], kPerm[pa][2]}, B{kPerm[pb][0], kPerm[pb][1], kPerm[pb][2]}, D{kPerm[pd][0], kPerm[pd][1], kPerm[pd][2]};
        // plain triple loop: D[blk][i][j] = C[blk][i][j] + sum_k A[blk][i][k] B[blk][j][k]
        double Am[4][4][4], Bm[4][4][4];
        for (int l = 0; l < 64; ++l) { Am[fld(l, A.blk)][fld(l, A.idx)][fld(l, A.k)] = ha[l]; Bm[fld(l, B.blk)][fld(l, B.idx)][fld(l, B.k)] = hb[l]; }
        bool ok = true;
        for (int l = 0; l < 64 && ok; ++l) {
          const int blk = fld(l, D.blk), i = fld(l, D.idx), j = fld(l, D.k);
          double s = hc[l];
          for (int k = 0; k < 4; ++k) s += Am[blk][i][k] * Bm[blk][j][k];
          ok = s == hd[l];
        }
        if (ok) {
          printf("  match: A lane = block<<%d | row<<%d | k<<%d   B lane = block<<%d | col<<%d | k<<%d   D lane = block<<%d | row<<%d | col<<%d\n",
                 A.blk, A.idx, A.k, B.blk, B.idx, B.k, D.blk, D.idx, D.k);
          if (!found) { fa = A; fb = B; fd = D; }
          ++found;
        }
      }
  if (!found) { printf("  no field layout reproduces the instruction: stop\n"); return 2; }
  if (probe_broadcast<0, 0>(dout, fa, fd) || probe_broadcast<1, 0>(dout, fa, fd) || probe_broadcast<1, 1>(dout, fa, fd) || probe_broadcast<2, 0>(dout, fa, fd) ||
      probe_broadcast<2, 1>(dout, fa, fd) || probe_broadcast<2, 2>(dout, fa, fd) || probe_broadcast<2, 3>(dout, fa, fd)) return 1;

  // ---- 2. cycles
  printf("2. cost (one wavefront per SIMD; clock64 ticks on one CU alone, then 256 CUs by event time)\n");
  double c[7];
  if (time_mode<0>("16x16x4, dependent chain (4 / iteration)", 4, dout, dcyc, &c[0])) return 1;
  if (time_mode<1>("16x16x4, 4 accumulators (4 / iteration)", 4, dout, dcyc, &c[1])) return 1;
  if (time_mode<2>("4x4x4 x 4 blocks, dependent chain (16 / iter.)", 16, dout, dcyc, &c[2])) return 1;
  if (time_mode<3>("4x4x4 x 4 blocks, 16 accumulators (16 / iter.)", 16, dout, dcyc, &c[3])) return 1;
  if (time_mode<4>("64 v_fma_f64", 64, dout, dcyc, &c[4])) return 1;
  if (time_mode<5>("16x16x4 stream + 64 v_fma_f64 interleaved", 0, dout, dcyc, &c[5])) return 1;
  if (time_mode<6>("4x4x4 stream + 64 v_fma_f64 interleaved", 0, dout, dcyc, &c[6])) return 1;
  printf("  four-block instruction / 16x16x4 instruction, independent streams: %.3f (a quarter = 0.25); dependent chains: %.3f\n", (c[3] / 16) / (c[1] / 4), (c[2] / 16) / (c[0] / 4));
  printf("  beside VALU: 16x16x4 %.1f (sum of the two alone %.1f), 4x4x4 %.1f (sum %.1f)\n", c[5], c[1] + c[4], c[6], c[3] + c[4]);

  // ---- 3. bits
  printf("3. bits: 16x16x4 against 4x4x4 blocks over the same k order\n");
  const int nimg = 256;
  std::vector<double> wa((size_t)nimg * kRows * kK), wb;
  for (int im = 0; im < nimg; ++im) {
    double* W = wa.data() + (size_t)im * kRows * kK;
    const int kind = im & 3;   // 0: uniform   1: column scales over 16 decades   2: rows in nearly opposite pairs   3: both
    for (int k = 0; k < kK; ++k) {
      const double cs = (kind & 1) ? std::pow(10.0, 16.0 * urand() - 8.0) : 1.0;
      for (int r = 0; r < kRows; ++r) {
        double x = (2.0 * urand() - 1.0) * cs;
        if ((kind & 2) && (k & 1)) x = -W[r * kK + k - 1] * (1.0 + 1e-13 * (urand() - 0.5) * (1 << (r & 7)));   // products cancel pairwise along k
        W[r * kK + k] = x;
      }
    }
  }
  wb = wa;
  for (int im = nimg / 2; im < nimg; ++im)   // second half: a different column image (cross items)
    for (int i = 0; i < kRows * kK; ++i) wb[(size_t)im * kRows * kK + i] = wa[(size_t)((im + 4) % nimg) * kRows * kK + (i * 5 + 3) % (kRows * kK)];
  double *dwa, *dwb, *dt, *dbk;
  CHECK(hipMalloc(&dwa, wa.size() * sizeof(double))); CHECK(hipMalloc(&dwb, wb.size() * sizeof(double)));
  CHECK(hipMalloc(&dt, (size_t)nimg * 256 * sizeof(double))); CHECK(hipMalloc(&dbk, (size_t)nimg * 256 * sizeof(double)));
  CHECK(hipMemcpy(dwa, wa.data(), wa.size() * sizeof(double), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(dwb, wb.data(), wb.size() * sizeof(double), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_bits_tile, dim3(nimg), dim3(64), 0, 0, dwa, dwb, dt, kK / 4);
  hipLaunchKernelGGL(k_bits_blocks, dim3(nimg), dim3(64), 0, 0, dwa, dwb, dbk, kK / 4, fa, fb, fd);
  CHECK(hipDeviceSynchronize());
  std::vector<double> ht((size_t)nimg * 256), hk((size_t)nimg * 256);
  CHECK(hipMemcpy(ht.data(), dt, ht.size() * sizeof(double), hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hk.data(), dbk, hk.size() * sizeof(double), hipMemcpyDeviceToHost));
  long long differ = 0, mirror_t = 0, mirror_b = 0, misplaced = 0, nonzero = 0;
  double worst = 0;
  for (int im = 0; im < nimg; ++im) {
    const double *A = wa.data() + (size_t)im * kRows * kK, *B = wb.data() + (size_t)im * kRows * kK;
    for (int r = 0; r < 16; ++r)
      for (int cc = 0; cc < 16; ++cc) {
        const double t = ht[(size_t)im * 256 + r * 16 + cc], b = hk[(size_t)im * 256 + r * 16 + cc];
        if (std::memcmp(&t, &b, 8)) { if (differ < 8) printf("  image %d (%d,%d): tile %.17g blocks %.17g\n", im, r, cc, t, b); ++differ; }
        if (im < nimg / 2) {
          const double tm = ht[(size_t)im * 256 + cc * 16 + r], bm = hk[(size_t)im * 256 + cc * 16 + r];
          mirror_t += std::memcmp(&t, &tm, 8) != 0; mirror_b += std::memcmp(&b, &bm, 8) != 0;
        }
        // the entry is the one the host's sum names (placement; loose, the summation order inside the instruction is not the host's)
        long double s = 0, mag = 0;
        for (int k = 0; k < kK; ++k) { s += (long double)A[r * kK + k] * B[cc * kK + k]; mag += fabsl((long double)A[r * kK + k] * B[cc * kK + k]); }
        const double err = (double)(fabsl(s - t) / (mag > 0 ? mag : 1));
        worst = err > worst ? err : worst;
        misplaced += err > 1e-13;
        nonzero += t != 0.0;
      }
  }
  printf("  %d images x 256 entries (%lld nonzero): %lld entries differ between tile and blocks; mirror (r,c) != (c,r): tile %lld, blocks %lld (symmetric half);\n"
         "  against the host's long double sum: worst |error| / sum |terms| = %.2e, %lld entries beyond 1e-13\n",
         nimg, nonzero, differ, mirror_t, mirror_b, worst, misplaced);
  if (differ || mirror_t || mirror_b || misplaced) { printf("  NOT identical: stop\n"); return 3; }
  printf("  identical bit for bit\n");
  return 0;
}
