// stereo_device.hip -- Frame::ComputeStereoMatches (src/Frame.cc:816-986) on MI355X (gfx950) for a batch of rectified stereo frames.
//
// Three kernels per call, every frame of the batch in each:
//   k_stereo_hamming  the row-band descriptor search (:833-899).  The reference's row table is not materialised: right keypoint iR is
//                     a candidate of left keypoint iL iff floor(yR - r) <= (int)vL <= ceil(yR + r), r = 2 * scale[octaveR], evaluated
//                     per pair in float32; the first minimum in ascending iR is the minimum of the packed key (distance << 22) | iR.
//   k_stereo_sad      one wavefront per left keypoint: the 11x11 left patch and the 11x21 right strip staged in LDS, the 11 sums of
//                     absolute differences, the first strict minimum, the parabola and the disparity tests (:902-969).
//   k_stereo_median   one block per frame: the size/2-th smallest accepted SAD by a two-pass radix select (SAD <= 121 * 255 < 2^15)
//                     and the cut at 1.5f * 1.4f * median (:972-985).
// Float32 steps are single IEEE operations in the reference's order, contraction off; `/` is the correctly rounded division.
//
// Three entries share the kernels and the host half (stereo_frame.h, stereo_match_on below); they differ in where the pixels are:
//   osh_orb_stereo_match           the caller brings both pyramids: the used levels are packed into the call's image arena;
//                                  the search is k_stereo_hamming, in the other two the row lists (k_stereo_rows_*, k_stereo_rowsearch);
//   osh_orb_stereo_match_resident  two frames of the context's resident pyramid, by token: StereoView::images is its first byte,
//                                  off_l / off_r the levels' offsets in it, nothing of the pyramids is staged or uploaded;
//   osh_orb_extract_stereo         the stereo match as the tail of osh_orb_extract(_raw) (orb_extract.h): k_stereo_level0 scales the
//                                  kept keypoints to level 0 where they lie, the descriptors are read where k_orb_brief left them,
//                                  the pixels in the resident pyramid the call has just built; its outputs join the one download.
#include "common.h"
#include "orb_extract.h"
#include "orb_hamming.h"
#include "orb_stage.h"
#include "stereo_frame.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr int kSBlock = 64;       // left keypoints per block of k_stereo_hamming (one per lane of one wavefront)
constexpr int kSTile = 256;       // right keypoints staged in LDS per tile: 8 KiB descriptors + 4 KiB predicate data
constexpr int kSadWaves = 4;      // left keypoints per block of k_stereo_sad (one per wavefront)
constexpr int kThHigh = 100, kThOrbDist = 75;   // ORBmatcher::TH_HIGH, (TH_HIGH + TH_LOW) / 2 (include/ORBmatcher.h, src/Frame.cc:821)

struct StereoView {
  int n_frames, n_split;
  const StereoFrameDev* frames;
  const float2* lxy; const int* loct; const uint4* ldesc;
  const float2* rxy; const int* roct; const uint4* rdesc;
  const unsigned char* images;
  unsigned* key;        // [NL] packed (distance << 22) | iR minimum, 0xFFFFFFFF none
  unsigned* rowhit;     // [NL] 1: the row of the left keypoint holds a right keypoint
  int* best_sad;        // [NL] bestDist of the SAD search for accepted keypoints
  float* u_right; float* depth; int* best_right; int* hamming; int* sad; int* best_inc; unsigned char* stage;
};

// grid = (ceil(max n_left / 64), n_frames, n_split); block z handles one slice of the right keypoints and merges by atomicMin
__global__ __launch_bounds__(kSBlock) void k_stereo_hamming(StereoView v) {
#pragma clang fp contract(off)
  __shared__ uint4 sh_desc[kSTile * 2];
  __shared__ int4 sh_pred[kSTile];   // minr, maxr, uR bits, octave
  const StereoFrameDev& f = v.frames[blockIdx.y];
  if ((int)blockIdx.x * kSBlock >= f.n_left) return;   // block-uniform
  const int iL = blockIdx.x * kSBlock + threadIdx.x;
  const bool valid = iL < f.n_left;
  const size_t gl = (size_t)f.left_base + (valid ? iL : 0);
  const float2 pl = v.lxy[gl];
  const int levelL = v.loct[gl];
  const uint4 a0 = v.ldesc[gl * 2], a1 = v.ldesc[gl * 2 + 1];
  const float maxD = f.bf / f.b;            // :848
  const float minU = pl.x - maxD;           // :866-867
  const float maxU = pl.x - 0.0f;
  const int row = (int)pl.y;                // vRowIndices[vL] (:861)
  const bool row_ok = valid && row >= 0 && row < f.n_rows;
  const int per = (f.n_right + (int)gridDim.z - 1) / (int)gridDim.z;
  const int t_begin = blockIdx.z * per, t_end = min(f.n_right, t_begin + per);
  unsigned best = 0xFFFFFFFFu;
  bool hit = false;
  for (int t0 = t_begin; t0 < t_end; t0 += kSTile) {
    const int nt = min(kSTile, t_end - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < nt * 2; k += kSBlock) sh_desc[k] = v.rdesc[((size_t)f.right_base + t0) * 2 + k];
    for (int k = threadIdx.x; k < nt; k += kSBlock) {
      const size_t gr = (size_t)f.right_base + t0 + k;
      const float2 pr = v.rxy[gr];
      const int octR = v.roct[gr];
      const float r = 2.0f * f.sf[octR];                 // :837-839
      const int maxr = (int)ceilf(pr.y + r);
      const int minr = (int)floorf(pr.y - r);
      sh_pred[k] = make_int4(minr, maxr, __float_as_int(pr.x), octR);
    }
    __syncthreads();
    for (int t = 0; t < nt; ++t) {
      const int4 p = sh_pred[t];                         // wave-wide broadcast read
      const bool in_row = row_ok && p.x <= row && row <= p.y;
      hit |= in_row;
      const float uR = __int_as_float(p.z);
      if (in_row && !(p.w < levelL - 1 || p.w > levelL + 1) && uR >= minU && uR <= maxU) {   // :883-888
        const unsigned d = hamming256(a0, a1, sh_desc[2 * t], sh_desc[2 * t + 1]);
        best = min(best, (d << kPosBits) | (unsigned)(t0 + t));
      }
    }
  }
  if (!valid) return;
  if (best != 0xFFFFFFFFu) atomicMin(&v.key[gl], best);
  if (hit) atomicOr(&v.rowhit[gl], 1u);
}

// ---- the row-list search of the entries that read resident pyramids: the reference's vRowIndices (:833-846) on the device.
// k_stereo_rows_enter (counting), k_stereo_rows_scan and k_stereo_rows_enter (filling) enter right keypoint iR into rows floor(y - r) .. ceil(y + r)
// clipped to [0, n_rows), r = 2 * scale[octave] in float32 (the statements of k_stereo_hamming's predicate): per-row counts, one
// exclusive prefix sum per frame, a fill through per-row cursors (integer atomics: the order inside a row does not enter the
// result).  k_stereo_rowsearch: one wavefront per left keypoint walks the list of its row, applies the level and [minU, maxU] gates
// and reduces the packed key by minimum: the minimum of the same keys over the same candidate set as k_stereo_hamming.
constexpr int kRowBlock = 256;
constexpr int kRowWaves = 4;      // left keypoints per block of k_stereo_rowsearch (one per wavefront)
struct StereoRowsView {
  const StereoRowsDev* frames;
  int* count;      // [rows of the batch] right keypoints entered into the row
  int* start;      // [rows] first entry of the row's list
  int* cursor;     // [rows] next free entry while the lists are filled
  int* entries;    // the lists: right keypoint indices inside their frame
};

__device__ __forceinline__ void stereo_row_span(const StereoFrameDev& f, float y, int octave, int& lo, int& hi) {
#pragma clang fp contract(off)
  const float r = 2.0f * f.sf[octave];                   // :837-839
  const int maxr = (int)ceilf(y + r);
  const int minr = (int)floorf(y - r);
  lo = max(minr, 0); hi = min(maxr, f.n_rows - 1);
}

// grid = (ceil(max n_right / 256), n_frames).  fill == 0: the counts; else the entries through the cursors
__global__ __launch_bounds__(kRowBlock) void k_stereo_rows_enter(StereoView v, StereoRowsView w, int fill) {
  const StereoFrameDev& f = v.frames[blockIdx.y];
  const StereoRowsDev R = w.frames[blockIdx.y];
  const int iR = blockIdx.x * kRowBlock + threadIdx.x;
  if (iR >= f.n_right) return;
  const size_t gr = (size_t)f.right_base + iR;
  int lo, hi;
  stereo_row_span(f, v.rxy[gr].y, v.roct[gr], lo, hi);
  for (int row = lo; row <= hi; ++row) {
    if (!fill) { atomicAdd(&w.count[R.row0 + row], 1); continue; }
    const int at = atomicAdd(&w.cursor[R.row0 + row], 1);
    if (at >= R.entry0 && at < R.entry_end) w.entries[at] = iR;   // the slice holds every entry by construction; never beyond it
  }
}

// grid = n_frames, block = 256: start = cursor = entry0 + the exclusive prefix sum of the frame's counts
__global__ __launch_bounds__(kRowBlock) void k_stereo_rows_scan(StereoView v, StereoRowsView w) {
  __shared__ int sh[kRowBlock];
  __shared__ int sh_carry;
  const StereoFrameDev& f = v.frames[blockIdx.x];
  const StereoRowsDev R = w.frames[blockIdx.x];
  const int tid = threadIdx.x;
  if (tid == 0) sh_carry = R.entry0;
  __syncthreads();
  for (int r0 = 0; r0 < f.n_rows; r0 += kRowBlock) {     // block-uniform
    const int row = r0 + tid;
    const int c = row < f.n_rows ? w.count[R.row0 + row] : 0;
    sh[tid] = c;
    __syncthreads();
    for (int d = 1; d < kRowBlock; d <<= 1) {            // inclusive scan of the chunk
      const int add = tid >= d ? sh[tid - d] : 0;
      __syncthreads();
      sh[tid] += add;
      __syncthreads();
    }
    const int first = sh_carry + sh[tid] - c;
    if (row < f.n_rows) { w.start[R.row0 + row] = first; w.cursor[R.row0 + row] = first; }
    __syncthreads();
    if (tid == kRowBlock - 1) sh_carry += sh[tid];
    __syncthreads();
  }
}

// grid = (ceil(max n_left / 4), n_frames), block = 4 wavefronts, one left keypoint each; writes key and rowhit of every left keypoint
__global__ __launch_bounds__(kRowWaves * 64) void k_stereo_rowsearch(StereoView v, StereoRowsView w) {
#pragma clang fp contract(off)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const StereoFrameDev& f = v.frames[blockIdx.y];
  const StereoRowsDev R = w.frames[blockIdx.y];
  const int iL = blockIdx.x * kRowWaves + wave;
  if (iL >= f.n_left) return;                            // wave-uniform; no barrier below
  const size_t gl = (size_t)f.left_base + iL;
  const float2 pl = v.lxy[gl];
  const int levelL = v.loct[gl];
  const uint4 a0 = v.ldesc[gl * 2], a1 = v.ldesc[gl * 2 + 1];
  const float maxD = f.bf / f.b;            // :848
  const float minU = pl.x - maxD;           // :866-867
  const float maxU = pl.x - 0.0f;
  const int row = (int)pl.y;                // vRowIndices[vL] (:861)
  int n = 0, first = 0;
  if (row >= 0 && row < f.n_rows) {
    first = w.start[R.row0 + row];
    n = min(w.count[R.row0 + row], R.entry_end - first);
  }
  unsigned best = 0xFFFFFFFFu;
  for (int k = lane; k < n; k += 64) {
    const int iR = w.entries[first + k];
    if ((unsigned)iR >= (unsigned)f.n_right) continue;   // cannot happen: every entry of a list was filled
    const size_t gr = (size_t)f.right_base + iR;
    const int octR = v.roct[gr];
    const float uR = v.rxy[gr].x;
    if (!(octR < levelL - 1 || octR > levelL + 1) && uR >= minU && uR <= maxU) {   // :883-888
      const unsigned d = hamming256(a0, a1, v.rdesc[gr * 2], v.rdesc[gr * 2 + 1]);
      best = min(best, (d << kPosBits) | (unsigned)iR);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, d, 64));
  if (lane == 0) { v.key[gl] = best; v.rowhit[gl] = n > 0 ? 1u : 0u; }
}

// round(): half away from zero (std::round of the reference, :907-909), not rint
__device__ __forceinline__ float round_away(float x) { return roundf(x); }

// grid = (ceil(max n_left / 4), n_frames), block = 4 wavefronts, one left keypoint each.  Every wavefront reaches every barrier.
__global__ __launch_bounds__(kSadWaves * 64) void k_stereo_sad(StereoView v) {
#pragma clang fp contract(off)
  __shared__ unsigned char sh_l[kSadWaves][11 * 11 + 3];
  __shared__ unsigned char sh_r[kSadWaves][11 * 21 + 1];
  __shared__ int sh_sad[kSadWaves][11];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const StereoFrameDev& f = v.frames[blockIdx.y];
  const int iL = blockIdx.x * kSadWaves + wave;
  const bool valid = iL < f.n_left;
  const size_t gl = (size_t)f.left_base + (valid ? iL : 0);
  int stage = -1, best_right = -1, ham = -1;
  int lvl = 0, su_l = 0, sv_l = 0, su_r = 0;
  float uL = 0.f;
  if (valid) {
    const float2 pl = v.lxy[gl];
    uL = pl.x;
    lvl = v.loct[gl];
    const unsigned key = v.key[gl];
    const bool has_row = v.rowhit[gl] != 0;
    const float maxU = pl.x - 0.0f;
    if (!has_row || maxU < 0) {                          // :863-870
      stage = OSH_STEREO_NO_CANDIDATE;
    } else {
      const unsigned d = key >> kPosBits;
      ham = kThHigh;
      if (key != 0xFFFFFFFFu && d < (unsigned)kThHigh) { ham = (int)d; best_right = (int)(key & kPosMask); }
      if (!(ham < kThOrbDist)) {                         // :902
        stage = OSH_STEREO_HAMMING;
      } else {
        const float uR0 = v.rxy[(size_t)f.right_base + best_right].x;
        const float isf = f.isf[lvl];
        const float scaleduL = round_away(pl.x * isf), scaledvL = round_away(pl.y * isf), scaleduR0 = round_away(uR0 * isf);   // :907-909
        const float iniu = scaleduR0 + 5.0f - 5.0f, endu = scaleduR0 + 5.0f + 5.0f + 1.0f;                                  // :921-922
        su_l = (int)scaleduL; sv_l = (int)scaledvL; su_r = (int)scaleduR0;
        if (iniu < 0 || endu >= (float)f.cols_r[lvl]) {  // :923
          stage = OSH_STEREO_RIGHT_GUARD;
        } else if (f.off_l[lvl] < 0 || f.off_r[lvl] < 0 || sv_l - 5 < 0 || sv_l + 5 >= f.rows_l[lvl] || sv_l + 5 >= f.rows_r[lvl] ||
                   su_l - 5 < 0 || su_l + 5 >= f.cols_l[lvl] || su_r - 10 < 0 || su_r + 10 >= f.cols_r[lvl]) {
          stage = OSH_STEREO_PATCH;                      // the reference reads outside the image here
        }
      }
    }
  }
  const bool search = valid && stage < 0;                // wave-uniform
  if (lane < 11) sh_sad[wave][lane] = 0;
  if (search) {
    const unsigned char* il = v.images + f.off_l[lvl] + (size_t)(sv_l - 5) * f.cols_l[lvl] + (su_l - 5);
    const unsigned char* ir = v.images + f.off_r[lvl] + (size_t)(sv_l - 5) * f.cols_r[lvl] + (su_r - 10);
    for (int k = lane; k < 121; k += 64) { const int r = k / 11, c = k - r * 11; sh_l[wave][k] = il[(size_t)r * f.cols_l[lvl] + c]; }
    for (int k = lane; k < 231; k += 64) { const int r = k / 21, c = k - r * 21; sh_r[wave][k] = ir[(size_t)r * f.cols_r[lvl] + c]; }
  }
  __syncthreads();
  if (search) {
    // item k = (increment i, patch row r): the 11 absolute differences of one row, added into the increment's sum (integers: any order)
    for (int k = lane; k < 121; k += 64) {
      const int i = k / 11, r = k - i * 11;
      const unsigned char* a = &sh_l[wave][r * 11];
      const unsigned char* b = &sh_r[wave][r * 21 + i];
      int s = 0;
#pragma unroll
      for (int c = 0; c < 11; ++c) s += abs((int)a[c] - (int)b[c]);
      atomicAdd(&sh_sad[wave][i], s);
    }
  }
  __syncthreads();
  if (!valid || lane != 0) return;
  int best_inc = OSH_STEREO_NO_INC;
  float u_right = -1.0f, depth = -1.0f;
  int sads[11];
#pragma unroll
  for (int i = 0; i < 11; ++i) sads[i] = search ? sh_sad[wave][i] : -1;
  if (search) {
    int best = INT_MAX, bi = 0;
#pragma unroll
    for (int i = 0; i < 11; ++i) if (sads[i] < best) { best = sads[i]; bi = i - 5; }   // :931-935, first strict minimum
    best_inc = bi;
    if (bi == -5 || bi == 5) {                           // :940
      stage = OSH_STEREO_BORDER_INC;
    } else {
      const float dist1 = (float)sh_sad[wave][5 + bi - 1], dist2 = (float)sh_sad[wave][5 + bi], dist3 = (float)sh_sad[wave][5 + bi + 1];
      const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));   // :948
      if (deltaR < -1 || deltaR > 1) {                   // :950
        stage = OSH_STEREO_DELTA;
      } else {
        const float sf = f.sf[lvl];
        float bestuR = sf * ((float)su_r + (float)bi + deltaR);    // :954
        float disparity = uL - bestuR;
        const float maxD = f.bf / f.b;
        if (disparity >= 0.0f && disparity < maxD) {     // :958
          if (disparity <= 0) {
            disparity = 0.01f;                           // (float)0.01
            bestuR = (float)((double)uL - 0.01);         // :963, double arithmetic, stored as float
          }
          depth = f.bf / disparity;                      // :965
          u_right = bestuR;
          stage = OSH_STEREO_ACCEPTED;
          v.best_sad[gl] = best;
        } else {
          stage = OSH_STEREO_DISPARITY;
        }
      }
    }
  }
  v.u_right[gl] = u_right; v.depth[gl] = depth;
  v.best_right[gl] = best_right; v.hamming[gl] = ham; v.best_inc[gl] = best_inc;
  v.stage[gl] = (unsigned char)stage;
#pragma unroll
  for (int i = 0; i < 11; ++i) v.sad[gl * 11 + i] = sads[i];
}

// grid = n_frames, block = 256.  Rank size/2 (0-based) of the accepted SADs: histogram of the high 8 bits, then of the low 7 bits
// inside the bin that holds the rank.
__global__ __launch_bounds__(256) void k_stereo_median(StereoView v) {
#pragma clang fp contract(off)
  __shared__ int sh_hist[256];
  __shared__ int sh_sel[2];   // selected bin, rank inside it
  const StereoFrameDev& f = v.frames[blockIdx.x];
  const size_t base = (size_t)f.left_base;
  const int tid = threadIdx.x;
  sh_hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < f.n_left; i += 256)
    if (v.stage[base + i] == OSH_STEREO_ACCEPTED) atomicAdd(&sh_hist[v.best_sad[base + i] >> 7], 1);
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int k = 0; k < 256; ++k) total += sh_hist[k];
    int bin = -1, rank = total / 2;                      // vDistIdx[vDistIdx.size() / 2] (:973)
    if (total > 0) {
      for (bin = 0; bin < 256; ++bin) { if (rank < sh_hist[bin]) break; rank -= sh_hist[bin]; }
    }
    sh_sel[0] = bin; sh_sel[1] = rank;
  }
  __syncthreads();
  const int bin = sh_sel[0], rank = sh_sel[1];
  if (bin < 0) return;                                   // no accepted keypoint: the reference indexes an empty vector here
  __syncthreads();
  sh_hist[tid] = 0;
  __syncthreads();
  for (int i = tid; i < f.n_left; i += 256)
    if (v.stage[base + i] == OSH_STEREO_ACCEPTED && (v.best_sad[base + i] >> 7) == bin) atomicAdd(&sh_hist[v.best_sad[base + i] & 127], 1);
  __syncthreads();
  if (tid == 0) {
    int r = rank, low = 0;
    for (; low < 128; ++low) { if (r < sh_hist[low]) break; r -= sh_hist[low]; }
    sh_sel[0] = (bin << 7) | low;
  }
  __syncthreads();
  const float median = (float)sh_sel[0];
  const float thDist = 1.5f * 1.4f * median;             // :974
  for (int i = tid; i < f.n_left; i += 256) {
    if (v.stage[base + i] != OSH_STEREO_ACCEPTED) continue;
    if (!((float)v.best_sad[base + i] < thDist)) {       // :978-984
      v.u_right[base + i] = -1.0f; v.depth[base + i] = -1.0f;
      v.stage[base + i] = OSH_STEREO_MEDIAN_CUT;
    }
  }
}

// The keypoints of the pairs as the kernels above read them, from the gathered keypoints of an extract (orb_extract.h): the
// write-back scaling of ORBextractor::operator() (src/ORBextractor.cc:1143-1150: `if (level != 0) pt *= scale`), one float32
// multiply per coordinate, and the octave.  levels: per level of the call its scale and its number inside its frame.
struct TailLevelDev { float scale; int octave; };
__global__ __launch_bounds__(256) void k_stereo_level0(int n, const float2* xy, const int* level_index, const TailLevelDev* levels, float2* sxy, int* octave) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const TailLevelDev L = levels[level_index[i]];
  float2 p = xy[i];
  if (L.octave != 0) { p.x = p.x * L.scale; p.y = p.y * L.scale; }
  sxy[i] = p;
  octave[i] = L.octave;
}

struct StereoState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
  int row_search = 1;   // of the entries on resident pyramids: 1 the row lists, 0 k_stereo_hamming (osh_orb_stereo_set_row_search)
};

// The row lists of a call: the plan of its frames (stereo_frame.h), its sections and their binding.  Not used (use == false) when
// the context asks for k_stereo_hamming or the lists are beyond the plan's sizes
struct StereoRowSections {
  StereoRowPlan plan;
  bool use = false;
  Section<StereoRowsDev> frames{0};
  Section<int> count{0}, start{0}, cursor{0}, entries{0};
  void take(bool wanted, const std::vector<StereoFrameDev>& fd, Layout& in, Layout& work) {
    for (const StereoFrameDev& d : fd) plan.add(d);
    use = wanted && plan.fits();
    if (!use) return;
    frames = in.take<StereoRowsDev>(plan.frames.size());
    count = work.take<int>(plan.rows); start = work.take<int>(plan.rows); cursor = work.take<int>(plan.rows);
    entries = work.take<int>(plan.entries);
  }
  void stage(char* h) const { if (use) std::memcpy(frames.in(h), plan.frames.data(), sizeof(StereoRowsDev) * plan.frames.size()); }
  StereoRowsView bind(char* di, char* dw) const { return StereoRowsView{frames.in(di), count.in(dw), start.in(dw), cursor.in(dw), entries.in(dw)}; }
};

// The outputs and the work arrays of NL left keypoints: sections of a call's layouts, their binding and their way back
struct StereoSections {
  Section<float> ur, depth;
  Section<int> br, ham, sad, inc;
  Section<unsigned char> stage;
  Section<unsigned> key, hit;
  Section<int> bsad;
  void take(size_t NL, Layout& out, Layout& work) {
    ur = out.take<float>(NL); depth = out.take<float>(NL);
    br = out.take<int>(NL); ham = out.take<int>(NL); sad = out.take<int>(NL * 11);
    inc = out.take<int>(NL); stage = out.take<unsigned char>(NL);
    key = work.take<unsigned>(NL); hit = work.take<unsigned>(NL); bsad = work.take<int>(NL);
  }
  void bind(StereoView& v, char* dout, char* dw) const {
    v.key = key.in(dw); v.rowhit = hit.in(dw); v.best_sad = bsad.in(dw);
    v.u_right = ur.in(dout); v.depth = depth.in(dout); v.best_right = br.in(dout); v.hamming = ham.in(dout);
    v.sad = sad.in(dout); v.best_inc = inc.in(dout); v.stage = stage.in(dout);
  }
  void scatter_to(const osh_stereo_result& r, const char* ho, size_t b, size_t n) const {
    scatter(r.u_right, ur, ho, b, n); scatter(r.depth, depth, ho, b, n);
    scatter(r.best_right, br, ho, b, n); scatter(r.hamming, ham, ho, b, n); scatter(r.sad, sad, ho, b, n, 11);
    scatter(r.best_inc, inc, ho, b, n); scatter(r.stage, stage, ho, b, n);
  }
};

// The three kernels over a bound view of NL > 0 left keypoints
static int stereo_launch(hipStream_t s, StereoView& v, size_t NL, int max_left, int max_right, const StereoRowSections* rows = nullptr, char* di = nullptr,
                         char* dw = nullptr) {
  const int n_frames = v.n_frames;
  if (rows && rows->use) {   // the row lists, then one wavefront per left keypoint on the list of its row
    const StereoRowsView w = rows->bind(di, dw);
    OSH_HIP(hipMemsetAsync(w.count, 0, rows->plan.rows * 4, s));
    if (max_right > 0) {
      const dim3 grid((unsigned)((max_right + kRowBlock - 1) / kRowBlock), (unsigned)n_frames);
      hipLaunchKernelGGL(k_stereo_rows_enter, grid, dim3(kRowBlock), 0, s, v, w, 0);
      hipLaunchKernelGGL(k_stereo_rows_scan, dim3((unsigned)n_frames), dim3(kRowBlock), 0, s, v, w);
      hipLaunchKernelGGL(k_stereo_rows_enter, grid, dim3(kRowBlock), 0, s, v, w, 1);
    }
    hipLaunchKernelGGL(k_stereo_rowsearch, dim3((unsigned)((max_left + kRowWaves - 1) / kRowWaves), (unsigned)n_frames), dim3(kRowWaves * 64), 0, s, v, w);
  } else {
    OSH_HIP(hipMemsetAsync(v.key, 0xFF, NL * 4, s));
    OSH_HIP(hipMemsetAsync(v.rowhit, 0, NL * 4, s));
    const int qblocks = (max_left + kSBlock - 1) / kSBlock;
    v.n_split = right_set_slices(qblocks, n_frames, max_right, kSTile);
    hipLaunchKernelGGL(k_stereo_hamming, dim3((unsigned)qblocks, (unsigned)n_frames, (unsigned)v.n_split), dim3(kSBlock), 0, s, v);
  }
  hipLaunchKernelGGL(k_stereo_sad, dim3((unsigned)((max_left + kSadWaves - 1) / kSadWaves), (unsigned)n_frames), dim3(kSadWaves * 64), 0, s, v);
  hipLaunchKernelGGL(k_stereo_median, dim3((unsigned)n_frames), dim3(256), 0, s, v);
  return launch_check("stereo match");
}

// The body of osh_orb_stereo_match and osh_orb_stereo_match_resident on validated frames.  plan(k, d, img_bytes) fills the level
// tables of frame k and grows the image arena by what the call uploads; stage_levels(arena, k, d) packs those levels.  resident:
// the base the offsets count from when nothing is uploaded (nullptr: the call's arena).
template <class Frame, class Plan, class StageLevels>
static int stereo_match_on(const char* entry, osh_orb_ctx* c, PhaseClock& clock, int n_frames, const Frame* frames, const osh_stereo_result* results,
                           const unsigned char* (*resident)(osh_orb_ctx*), Plan&& plan, StageLevels&& stage_levels) {
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  StereoState* st = orb_state<StereoState>(c, kOrbAttachStereo);
  clock.profiling = orb_profiling(c);

  // sizes: keypoints of the batch one frame after another; the image arena holds the used levels, rows packed
  KeypointBatch kb;
  OSH_TRY(kb.size(entry, n_frames, frames));
  const size_t NL = kb.NL;
  size_t img_bytes = 0;
  std::vector<StereoFrameDev> fd(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const Frame& f = frames[k];
    fd[k] = stereo_frame_dev(f.n_left, f.n_right, kb.base[k].left, kb.base[k].right, f.n_levels, f.bf, f.b, f.scale_factors, f.inv_scale_factors);
    plan(k, fd[k], img_bytes);
  }
  Layout in, out, work;
  const auto s_frames = in.take<StereoFrameDev>(n_frames);
  kb.take(in);
  const auto s_img = in.take<unsigned char>(img_bytes);
  StereoSections o;
  o.take(NL, out, work);
  StereoRowSections rows;
  rows.take(resident != nullptr && st->row_search != 0, fd, in, work);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  std::memcpy(s_frames.in(h), fd.data(), sizeof(StereoFrameDev) * n_frames);
  kb.stage(h, frames);
  rows.stage(h);
  for (int k = 0; k < n_frames; ++k) stage_levels(s_img.in(h), k, fd[k]);
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  if (NL) {
    StereoView v{};
    char* di = st->call.dev_in();
    v.n_frames = n_frames;
    v.frames = s_frames.in(di);
    kb.bind(v, di);
    v.images = resident ? resident(c) : s_img.in(di);
    o.bind(v, st->call.dev_out(), st->call.dev_work());
    OSH_TRY(stereo_launch(s, v, NL, kb.max_left, kb.max_right, &rows, di, st->call.dev_work()));
  }
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_frames; ++k) o.scatter_to(results[k], ho, (size_t)kb.base[k].left, (size_t)frames[k].n_left);
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

static const unsigned char* resident_images(osh_orb_ctx* c) { return orb_state<FastState>(c, kOrbAttachFast)->pyramid.images(); }

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_stereo_match(osh_orb_ctx* c, int32_t n_frames, const osh_stereo_frame* frames, const osh_stereo_result* results) {
  if (!c || n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_stereo_match: bad arguments"); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  PhaseClock clock;
  for (int k = 0; k < n_frames; ++k) OSH_TRY(stereo_validate_frame<BroughtStereoLevels>(k, frames[k], results[k], kPosMask));
  return stereo_match_on("osh_orb_stereo_match", c, clock, n_frames, frames, results, nullptr,
                         [&](int k, StereoFrameDev& d, size_t& img_bytes) { stereo_plan_brought(frames[k], d, img_bytes); },
                         [&](unsigned char* arena, int k, const StereoFrameDev& d) {
                           for (int l = 0; l < frames[k].n_levels; ++l) {
                             if (d.off_l[l] < 0) continue;
                             pack_level(arena + d.off_l[l], frames[k].left_pyramid[l]);
                             pack_level(arena + d.off_r[l], frames[k].right_pyramid[l]);
                           }
                         });
}

extern "C" int osh_orb_stereo_match_resident(osh_orb_ctx* c, int32_t n_frames, const osh_stereo_resident_frame* frames, const osh_stereo_result* results) {
  const char* entry = "osh_orb_stereo_match_resident";
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  PhaseClock clock;
  for (int k = 0; k < n_frames; ++k) OSH_TRY(stereo_validate_frame<ResidentStereoLevels>(k, frames[k], results[k], kPosMask));   // needs no context and no device
  if (!c) { set_error("%s: no context", entry); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  const PyramidTable& table = orb_state<FastState>(c, kOrbAttachFast)->pyramid;   // read only: the resident pyramid stays as it is
  std::vector<const FastFrameHost*> L(n_frames), R(n_frames);
  for (int k = 0; k < n_frames; ++k) OSH_TRY(stereo_check_tokens(entry, k, &table, frames[k].left_token, frames[k].right_token, frames[k].n_levels, &L[k], &R[k]));
  return stereo_match_on(entry, c, clock, n_frames, frames, results, resident_images,
                         [&](int k, StereoFrameDev& d, size_t&) { stereo_plan_resident(table, *L[k], *R[k], d); },
                         [](unsigned char*, int, const StereoFrameDev&) {});
}

extern "C" int osh_orb_stereo_set_row_search(osh_orb_ctx* c, int32_t enable) {
  if (!c) { set_error("osh_orb_stereo_set_row_search: bad arguments"); return OSH_ERR_INVALID; }
  orb_state<StereoState>(c, kOrbAttachStereo)->row_search = enable ? 1 : 0;
  return OSH_OK;
}

extern "C" int osh_orb_stereo_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<StereoState>("osh_orb_stereo_get_times", c, kOrbAttachStereo, ms);
}

extern "C" int osh_orb_extract_stereo(osh_orb_ctx* c, int32_t n_pairs, const osh_prepare_frame* prepare_frames, const osh_extract_frame* extract_frames,
                                      const osh_stereo_pair* pairs, osh_extract_result* extract_results, const osh_stereo_result* stereo_results) {
  const char* entry = "osh_orb_extract_stereo";
  if (n_pairs < 0 || (n_pairs && (!extract_frames || !extract_results))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  if (n_pairs && (!pairs || !stereo_results)) { set_error("%s: NULL pairs or stereo_results", entry); return OSH_ERR_INVALID; }
  if (n_pairs > 32767) { set_error("%s: more than 32767 pairs in one call", entry); return OSH_ERR_UNSUPPORTED; }
  for (int p = 0; p < n_pairs; ++p) {
    const osh_stereo_pair& q = pairs[p];
    if (!(q.b > 0.f) || !std::isfinite(q.bf) || !std::isfinite(q.b)) { set_error("%s: pair %d: bad bf / b", entry, p); return OSH_ERR_INVALID; }
    if (extract_frames[2 * p].n_levels != extract_frames[2 * p + 1].n_levels) {
      set_error("%s: pair %d: the left frame has %d levels, the right frame %d", entry, p, extract_frames[2 * p].n_levels, extract_frames[2 * p + 1].n_levels);
      return OSH_ERR_INVALID;
    }
    if (extract_results[2 * p].capacity > 0 && (!stereo_results[p].u_right || !stereo_results[p].depth)) {
      set_error("%s: pair %d: NULL u_right or depth with a left capacity of %d", entry, p, extract_results[2 * p].capacity); return OSH_ERR_INVALID;
    }
  }
  const int n_frames = 2 * n_pairs;

  // the tail: the left frames' keypoints first (pair after pair), then the right frames', so that each side is one array of the kernels
  ExtractTail tail;
  for (int side = 0; side < 2; ++side)
    for (int p = 0; p < n_pairs; ++p) tail.order.push_back(2 * p + side);
  std::vector<StereoFrameDev> fd((size_t)n_pairs);
  std::vector<TailLevelDev> tl;
  std::vector<size_t> left_n((size_t)n_pairs);
  Section<StereoFrameDev> s_frames{0};
  Section<TailLevelDev> s_levels{0};
  Section<float2> w_sxy{0};
  Section<int> w_oct{0};
  StereoSections o;
  StereoRowSections rows;
  const bool row_search = c && orb_state<StereoState>(c, kOrbAttachStereo)->row_search != 0;
  size_t NL = 0;
  int max_left = 0, max_right = 0;
  tail.plan = [&](const FastEmitted& e, const std::vector<size_t>& kp0, const std::vector<size_t>& n, Layout& in, Layout& out, Layout& work) {
    NL = 0; max_left = max_right = 0;
    for (int p = 0; p < n_pairs; ++p) NL += n[2 * p];
    tl.resize(e.levels.size());
    for (int p = 0; p < n_pairs; ++p) {
      const int l = 2 * p, r = 2 * p + 1;
      const osh_extract_frame& f = extract_frames[l];
      if (n[r] > (size_t)kPosMask) { set_error("%s: pair %d: n_right exceeds %u", entry, p, kPosMask); return (int)OSH_ERR_UNSUPPORTED; }
      StereoFrameDev& d = fd[p];
      d = stereo_frame_dev((int)n[l], (int)n[r], (int)kp0[l], (int)(kp0[r] - NL), f.n_levels, pairs[p].bf, pairs[p].b, f.scale, f.inv_scale);
      d.n_rows = e.levels[e.level0[l]].rows;
      for (int v = 0; v < f.n_levels; ++v) {
        const EmittedLevel& a = e.levels[e.level0[l] + v];
        const EmittedLevel& b = e.levels[e.level0[r] + v];
        d.rows_l[v] = a.rows; d.cols_l[v] = a.cols; d.off_l[v] = a.img_off;
        d.rows_r[v] = b.rows; d.cols_r[v] = b.cols; d.off_r[v] = b.img_off;
        tl[e.level0[l] + v] = {extract_frames[l].scale[v], v};
        tl[e.level0[r] + v] = {extract_frames[r].scale[v], v};
      }
      left_n[p] = n[l];
      // a frame whose arrays do not fit is not written, and neither are the stereo arrays of its pair
      if (n[l] > (size_t)extract_results[l].capacity || n[r] > (size_t)extract_results[r].capacity) left_n[p] = 0;
      max_left = std::max(max_left, (int)n[l]); max_right = std::max(max_right, (int)n[r]);
    }
    s_frames = in.take<StereoFrameDev>((size_t)n_pairs);
    s_levels = in.take<TailLevelDev>(tl.size());
    o.take(NL, out, work);
    rows.take(row_search, fd, in, work);
    size_t K = 0;
    for (int k = 0; k < n_frames; ++k) K += n[k];
    w_sxy = work.take<float2>(K); w_oct = work.take<int>(K);
    return (int)OSH_OK;
  };
  tail.stage = [&](char* h) {
    std::memcpy(s_frames.in(h), fd.data(), sizeof(StereoFrameDev) * fd.size());
    std::memcpy(s_levels.in(h), tl.data(), sizeof(TailLevelDev) * tl.size());
    rows.stage(h);
  };
  tail.launch = [&](hipStream_t s, char* di, char* dout, char* dw, const ExtractKept& kept) {
    if (!NL) return (int)OSH_OK;   // no left keypoint: nothing to match and nothing to write
    hipLaunchKernelGGL(k_stereo_level0, dim3((unsigned)((kept.K + 255) / 256)), dim3(256), 0, s, (int)kept.K, kept.xy, kept.level_index, s_levels.in(di),
                       w_sxy.in(dw), w_oct.in(dw));
    StereoView v{};
    v.n_frames = n_pairs;
    v.frames = s_frames.in(di);
    // desc is 256-byte aligned and a descriptor is 32 bytes: every keypoint's two uint4 are aligned, the right side's too
    v.lxy = w_sxy.in(dw); v.loct = w_oct.in(dw); v.ldesc = reinterpret_cast<const uint4*>(kept.desc);
    v.rxy = v.lxy + NL; v.roct = v.loct + NL; v.rdesc = v.ldesc + 2 * NL;
    v.images = kept.images;
    o.bind(v, dout, dw);
    return stereo_launch(s, v, NL, max_left, max_right, &rows, di, dw);
  };
  tail.collect = [&](const char* ho) {
    for (int p = 0; p < n_pairs; ++p) o.scatter_to(stereo_results[p], ho, (size_t)fd[p].left_base, left_n[p]);
  };
  return prepare_frames ? extract_raw_from(entry, c, n_frames, prepare_frames, extract_frames, extract_results, nullptr, &tail)
                        : extract_from(entry, c, n_frames, extract_frames, extract_results, nullptr, &tail);
}


