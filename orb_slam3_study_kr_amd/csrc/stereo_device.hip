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
#include "common.h"
#include "orb_hamming.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr int kSBlock = 64;       // left keypoints per block of k_stereo_hamming (one per lane of one wavefront)
constexpr int kSTile = 256;       // right keypoints staged in LDS per tile: 8 KiB descriptors + 4 KiB predicate data
constexpr int kSadWaves = 4;      // left keypoints per block of k_stereo_sad (one per wavefront)
constexpr int kThHigh = 100, kThOrbDist = 75;   // ORBmatcher::TH_HIGH, (TH_HIGH + TH_LOW) / 2 (include/ORBmatcher.h, src/Frame.cc:821)

struct StereoFrameDev {
  int n_left, n_right, left_base, right_base;   // bases: offsets of this frame in the keypoint arrays of the batch
  int n_rows;                                   // mvImagePyramid[0].rows of the left extractor
  int n_levels;
  float bf, b;
  float sf[OSH_STEREO_MAX_LEVELS], isf[OSH_STEREO_MAX_LEVELS];
  int rows_l[OSH_STEREO_MAX_LEVELS], cols_l[OSH_STEREO_MAX_LEVELS], rows_r[OSH_STEREO_MAX_LEVELS], cols_r[OSH_STEREO_MAX_LEVELS];
  long long off_l[OSH_STEREO_MAX_LEVELS], off_r[OSH_STEREO_MAX_LEVELS];   // byte offsets in the image arena (rows packed, stride = cols); -1: not uploaded
};

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


struct StereoState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

static int stereo_validate(int n_frames, const osh_stereo_frame* frames, const osh_stereo_result* results) {
  for (int k = 0; k < n_frames; ++k) {
    const osh_stereo_frame& f = frames[k];
    const osh_stereo_result& r = results[k];
    if (f.n_left < 0 || f.n_right < 0) { set_error("frame %d: negative keypoint count", k); return OSH_ERR_INVALID; }
    OSH_TRY(validate_keypoint_sides(k, f, kPosMask));
    if (!f.scale_factors || !f.inv_scale_factors || !f.left_pyramid || !f.right_pyramid) { set_error("frame %d: NULL scale factors or pyramid", k); return OSH_ERR_INVALID; }
    if (f.n_left && (!f.left_xy || !f.left_octave || !f.left_desc || !r.u_right || !r.depth)) { set_error("frame %d: NULL left keypoint or result array", k); return OSH_ERR_INVALID; }
    if (f.n_right && (!f.right_xy || !f.right_octave || !f.right_desc)) { set_error("frame %d: NULL right keypoint array", k); return OSH_ERR_INVALID; }
    if (!(f.b > 0.f) || !std::isfinite(f.bf) || !std::isfinite(f.b)) { set_error("frame %d: bad bf / b", k); return OSH_ERR_INVALID; }
    if (f.left_pyramid[0].rows <= 0) { set_error("frame %d: left_pyramid[0].rows must be positive", k); return OSH_ERR_INVALID; }
    auto coords_ok = [](const float* xy, int n) {
      for (int i = 0; i < 2 * n; ++i) if (!(std::fabs(xy[i]) <= OSH_STEREO_MAX_COORD)) return false;   // NaN fails too
      return true;
    };
    if (!coords_ok(f.left_xy, f.n_left) || !coords_ok(f.right_xy, f.n_right)) { set_error("frame %d: keypoint coordinate not finite or beyond %g", k, (double)OSH_STEREO_MAX_COORD); return OSH_ERR_INVALID; }
    OSH_TRY(validate_octaves(k, "right", f.right_octave, f.n_right, f.n_levels));
    for (int i = 0; i < f.n_left; ++i) {   // octave and image keypoint by keypoint: not validate_octaves, which would test every octave first
      const int o = f.left_octave[i];
      if (o < 0 || o >= f.n_levels) { set_error("frame %d: left octave %d outside [0, %d)", k, o, f.n_levels); return OSH_ERR_INVALID; }
      const osh_stereo_image* im[2] = {&f.left_pyramid[o], &f.right_pyramid[o]};
      for (int s = 0; s < 2; ++s)
        if (!im[s]->data || im[s]->rows <= 0 || im[s]->cols <= 0 || im[s]->stride < im[s]->cols) {
          set_error("frame %d: level %d (%s) is used by a left keypoint but its image is NULL, empty or has stride < cols", k, o, s ? "right" : "left");
          return OSH_ERR_INVALID;
        }
    }
  }
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_stereo_match(osh_orb_ctx* c, int32_t n_frames, const osh_stereo_frame* frames, const osh_stereo_result* results) {
  if (!c || n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_stereo_match: bad arguments"); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  PhaseClock clock;
  OSH_TRY(stereo_validate(n_frames, frames, results));
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  StereoState* st = orb_state<StereoState>(c, kOrbAttachStereo);
  clock.profiling = orb_profiling(c);

  // sizes: keypoints of the batch one frame after another; the image arena holds the used levels, rows packed
  KeypointBatch kb;
  OSH_TRY(kb.size("osh_orb_stereo_match", n_frames, frames));
  const size_t NL = kb.NL;
  size_t img_bytes = 0;
  std::vector<StereoFrameDev> fd(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const osh_stereo_frame& f = frames[k];
    StereoFrameDev& d = fd[k];
    std::memset(&d, 0, sizeof d);
    d.n_left = f.n_left; d.n_right = f.n_right; d.left_base = kb.base[k].left; d.right_base = kb.base[k].right;
    d.n_rows = f.left_pyramid[0].rows; d.n_levels = f.n_levels; d.bf = f.bf; d.b = f.b;
    bool used[OSH_STEREO_MAX_LEVELS] = {false};
    for (int i = 0; i < f.n_left; ++i) used[f.left_octave[i]] = true;
    for (int l = 0; l < OSH_STEREO_MAX_LEVELS; ++l) { d.off_l[l] = d.off_r[l] = -1; d.sf[l] = d.isf[l] = 1.f; }
    for (int l = 0; l < f.n_levels; ++l) {
      d.sf[l] = f.scale_factors[l]; d.isf[l] = f.inv_scale_factors[l];
      d.rows_l[l] = f.left_pyramid[l].rows; d.cols_l[l] = f.left_pyramid[l].cols;
      d.rows_r[l] = f.right_pyramid[l].rows; d.cols_r[l] = f.right_pyramid[l].cols;
      if (!used[l]) continue;
      d.off_l[l] = (long long)img_bytes; img_bytes += (size_t)d.rows_l[l] * d.cols_l[l];
      d.off_r[l] = (long long)img_bytes; img_bytes += (size_t)d.rows_r[l] * d.cols_r[l];
    }
  }
  Layout in, out, work;
  const auto s_frames = in.take<StereoFrameDev>(n_frames);
  kb.take(in);
  const auto s_img = in.take<unsigned char>(img_bytes);
  const auto o_ur = out.take<float>(NL); const auto o_depth = out.take<float>(NL);
  const auto o_br = out.take<int>(NL); const auto o_ham = out.take<int>(NL); const auto o_sad = out.take<int>(NL * 11);
  const auto o_inc = out.take<int>(NL); const auto o_stage = out.take<unsigned char>(NL);
  const auto w_key = work.take<unsigned>(NL); const auto w_hit = work.take<unsigned>(NL); const auto w_bsad = work.take<int>(NL);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  std::memcpy(s_frames.in(h), fd.data(), sizeof(StereoFrameDev) * n_frames);
  kb.stage(h, frames);
  for (int k = 0; k < n_frames; ++k) {
    const osh_stereo_frame& f = frames[k];
    const StereoFrameDev& d = fd[k];
    for (int l = 0; l < f.n_levels; ++l) {
      if (d.off_l[l] < 0) continue;
      const osh_stereo_image* im[2] = {&f.left_pyramid[l], &f.right_pyramid[l]};
      const long long off[2] = {d.off_l[l], d.off_r[l]};
      for (int side = 0; side < 2; ++side) pack_level(s_img.in(h) + off[side], *im[side]);
    }
  }
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  if (NL) {
    StereoView v{};
    char* di = st->call.dev_in(); char* dout = st->call.dev_out(); char* dw = st->call.dev_work();
    v.n_frames = n_frames;
    v.frames = s_frames.in(di);
    kb.bind(v, di);
    v.images = s_img.in(di);
    v.key = w_key.in(dw); v.rowhit = w_hit.in(dw); v.best_sad = w_bsad.in(dw);
    v.u_right = o_ur.in(dout); v.depth = o_depth.in(dout); v.best_right = o_br.in(dout); v.hamming = o_ham.in(dout);
    v.sad = o_sad.in(dout); v.best_inc = o_inc.in(dout); v.stage = o_stage.in(dout);
    OSH_HIP(hipMemsetAsync(v.key, 0xFF, NL * 4, s));
    OSH_HIP(hipMemsetAsync(v.rowhit, 0, NL * 4, s));
    const int qblocks = (kb.max_left + kSBlock - 1) / kSBlock;
    v.n_split = right_set_slices(qblocks, n_frames, kb.max_right, kSTile);
    hipLaunchKernelGGL(k_stereo_hamming, dim3((unsigned)qblocks, (unsigned)n_frames, (unsigned)v.n_split), dim3(kSBlock), 0, s, v);
    hipLaunchKernelGGL(k_stereo_sad, dim3((unsigned)((kb.max_left + kSadWaves - 1) / kSadWaves), (unsigned)n_frames), dim3(kSadWaves * 64), 0, s, v);
    hipLaunchKernelGGL(k_stereo_median, dim3((unsigned)n_frames), dim3(256), 0, s, v);
    OSH_TRY(launch_check("stereo match"));
  }
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  for (int k = 0; k < n_frames; ++k) {
    const osh_stereo_result& r = results[k];
    const size_t n = (size_t)frames[k].n_left, b = (size_t)kb.base[k].left;
    scatter(r.u_right, o_ur, ho, b, n); scatter(r.depth, o_depth, ho, b, n);
    scatter(r.best_right, o_br, ho, b, n); scatter(r.hamming, o_ham, ho, b, n); scatter(r.sad, o_sad, ho, b, n, 11);
    scatter(r.best_inc, o_inc, ho, b, n); scatter(r.stage, o_stage, ho, b, n);
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_stereo_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<StereoState>("osh_orb_stereo_get_times", c, kOrbAttachStereo, ms);
}
