// orb_fast_device.hip -- the integer part of ORBextractor::ComputeKeyPointsOctTree (src/ORBextractor.cc:781-896) on MI355X (gfx950)
// for a batch of pyramids: the cell-wise FAST-9/16 corners that go into DistributeOctTree and IC_Angle.  The statements are those of
// orb_fast.h.
//
// osh_orb_fast_detect, every cell of every level of every frame in each kernel:
//   k_fast_cells   one block per cell, largest cells first: the sub-image (at most 75 x 75 bytes) into LDS, the score map as bytes
//                  beside it, the 3x3 strict-maximum test, and per wavefront one ballot per 64 pixels at each threshold.  The block
//                  leaves the kept-corner bit mask of the threshold the cell is decided at (row-major, one bit per pixel), its
//                  count and how it was decided.  No atomic: every word of the mask is one wavefront's ballot.
//   k_fast_scan    one block: the exclusive scan of the counts over the cells in (frame, level, i, j) order.
//   k_fast_emit    one wavefront per cell: the set bits of the mask in ascending order at offset[cell] + rank, the score of each
//                  read again from the packed level.
// The host reads the offsets between scan and emit: they size the output.  Where a result lands is a function of the counts alone.
// fast_emit is the detector up to there: the candidates stay in the context's emit buffer; fast_download brings them to the host for
// the two detect entries, and osh_orb_extract (orb_extract_device.hip) leaves them where they are (fast_emit_resident, orb_extract.h).
//
// osh_orb_ic_angle: k_ic_angle, one keypoint per lane, reads its 31-pixel disc from the packed level.
#include "common.h"
#include "orb_extract.h"
#include "orb_fast.h"
#include "orb_pyramid_set.h"
#include "orb_stage.h"
#include <cmath>
#include <numeric>
#include <vector>

namespace osh {

constexpr int kFcBlock = 256;                       // k_fast_cells: 4 wavefronts
constexpr int kFcImgPitch = kFastMaxCell + 1;       // 76
constexpr int kFcScorePitch = kFastMaxCell + 2;     // 77: one pixel of zeros around the map
constexpr int kFcRounds = (kFastMaxCell * kFastMaxCell + kFcBlock - 1) / kFcBlock;   // 22
constexpr int kFeWords = (kFastMaskWords + 63) / 64;                                  // mask words per lane of k_fast_emit: 3
constexpr int kScanBlock = 256;
constexpr int kIcBlock = 64;

struct FastCellDev {
  long long img_off;       // first pixel of the level in the image arena (rows packed)
  int cols;                // of the level
  int x0, y0, w, h;        // the sub-image
  int shift_x, shift_y;    // j * wCell, i * hCell
  int level, cell;         // cell: number inside its frame
  int ini_th, min_th;
};

struct FastView {
  int n_cells;
  const FastCellDev* cells;     // (frame, level, i, j) order
  const int* order;             // launch order: largest sub-image first
  const unsigned char* images;
  unsigned* mask;               // [n_cells * kFastMaskWords]
  int* count;                   // [n_cells]
  int* offset;                  // [n_cells + 1]
  unsigned char* used_min;      // [n_cells]
  float2* xy; float* response; int* level; int* cell;   // [total]
};

__global__ __launch_bounds__(kFcBlock) void k_fast_cells(FastView v) {
  __shared__ unsigned char sh_img[kFastMaxCell * kFcImgPitch];
  __shared__ unsigned char sh_score[kFcScorePitch * kFcScorePitch];
  __shared__ unsigned sh_mask[2][kFcRounds * (kFcBlock / 32)];
  __shared__ int sh_cnt[2][kFcBlock / 64];
  const int c = v.order[blockIdx.x];
  const FastCellDev& cd = v.cells[c];
  const int w = cd.w, h = cd.h, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned char* src = v.images + cd.img_off + (size_t)cd.y0 * cd.cols + cd.x0;
  // one pixel per thread and round, with a division: a row per wavefront avoids it but was measured slower (93 VGPR against 64)
  for (int k = tid; k < w * h; k += kFcBlock) { const int y = k / w, x = k - y * w; sh_img[y * kFcImgPitch + x] = src[(size_t)y * cd.cols + x]; }
  for (int k = tid; k < kFcScorePitch * kFcScorePitch; k += kFcBlock) sh_score[k] = 0;
  __syncthreads();
  const int wi = w - 6, hi = h - 6;   // scores exist for rows and columns [3, size - 3)
  if (wi > 0 && hi > 0)
    for (int k = tid; k < wi * hi; k += kFcBlock) {
      const int y = 3 + k / wi, x = 3 + k % wi;
      sh_score[(y + 1) * kFcScorePitch + x + 1] = (unsigned char)fast_score_at(&sh_img[y * kFcImgPitch + x], kFcImgPitch);
    }
  __syncthreads();
  int n_ini = 0, n_min = 0;   // of this wavefront (the same in every lane)
  const int rounds = (w * h + kFcBlock - 1) / kFcBlock;
  for (int r = 0; r < rounds; ++r) {
    const int k = r * kFcBlock + tid;
    bool at_ini = false, at_min = false;
    if (k < w * h) {
      const int y = k / w, x = k - y * w;
      const unsigned char* s = &sh_score[(y + 1) * kFcScorePitch + x + 1];
      const bool kept = fast_is_kept(s, kFcScorePitch);
      at_ini = kept && s[0] >= cd.ini_th; at_min = kept && s[0] >= cd.min_th;
    }
    const unsigned long long b_ini = __ballot(at_ini), b_min = __ballot(at_min);
    n_ini += __popcll(b_ini); n_min += __popcll(b_min);
    if (lane < 2) {
      const int word = r * (kFcBlock / 32) + wave * 2 + lane;
      sh_mask[0][word] = (unsigned)(b_ini >> (32 * lane)); sh_mask[1][word] = (unsigned)(b_min >> (32 * lane));
    }
  }
  if (lane == 0) { sh_cnt[0][wave] = n_ini; sh_cnt[1][wave] = n_min; }
  __syncthreads();
  int t_ini = 0, t_min = 0;
  for (int k = 0; k < kFcBlock / 64; ++k) { t_ini += sh_cnt[0][k]; t_min += sh_cnt[1][k]; }
  const int which = t_ini ? 0 : 1;                      // :843: the second threshold only for a cell without corners at the first
  const int words = (w * h + 31) / 32;                  // <= rounds * 8
  for (int k = tid; k < words; k += kFcBlock) v.mask[(size_t)c * kFastMaskWords + k] = sh_mask[which][k];
  if (tid == 0) {
    v.count[c] = t_ini ? t_ini : t_min;
    v.used_min[c] = (unsigned char)(t_ini ? kFastAtIni : t_min ? kFastAtMin : kFastEmpty);
  }
}

// offset[c] = count[0] + ... + count[c - 1], offset[n_cells] = the total.  One block; every thread sums a run of cells.
__global__ __launch_bounds__(kScanBlock) void k_fast_scan(FastView v) {
  __shared__ int sh[kScanBlock];
  const int tid = threadIdx.x;
  const int per = (v.n_cells + kScanBlock - 1) / kScanBlock;
  const int begin = min(v.n_cells, tid * per), end = min(v.n_cells, begin + per);
  int sum = 0;
  for (int c = begin; c < end; ++c) sum += v.count[c];
  sh[tid] = sum;
  __syncthreads();
  for (int step = 1; step < kScanBlock; step <<= 1) {
    const int add = tid >= step ? sh[tid - step] : 0;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  int run = sh[tid] - sum;
  for (int c = begin; c < end; ++c) { v.offset[c] = run; run += v.count[c]; }
  if (tid == kScanBlock - 1) v.offset[v.n_cells] = sh[tid];
}

// One wavefront per cell; lane l owns the mask words [3 l, 3 l + 3), so ranks ascend with the lane and inside it with the bit.
__global__ __launch_bounds__(64) void k_fast_emit(FastView v) {
  const int c = blockIdx.x, lane = threadIdx.x;
  if (v.count[c] == 0) return;
  const FastCellDev& cd = v.cells[c];
  const int words = (cd.w * cd.h + 31) / 32;
  unsigned m[kFeWords];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < kFeWords; ++k) {
    const int word = lane * kFeWords + k;
    m[k] = word < words ? v.mask[(size_t)c * kFastMaskWords + word] : 0u;
    mine += __popc(m[k]);
  }
  int incl = mine;
#pragma unroll
  for (int step = 1; step < 64; step <<= 1) { const int up = __shfl_up(incl, step); if (lane >= step) incl += up; }
  int at = v.offset[c] + incl - mine;
  const unsigned char* lvl = v.images + cd.img_off;
#pragma unroll
  for (int k = 0; k < kFeWords; ++k) {
    unsigned bits = m[k];
    while (bits) {
      const int b = __ffs(bits) - 1;
      bits &= bits - 1;
      const int pix = (lane * kFeWords + k) * 32 + b;
      const int y = pix / cd.w, x = pix - y * cd.w;
      const int s = fast_score_at(lvl + (size_t)(cd.y0 + y) * cd.cols + cd.x0 + x, cd.cols);
      v.xy[at] = make_float2((float)(x + cd.shift_x), (float)(y + cd.shift_y));
      v.response[at] = (float)s; v.level[at] = cd.level; v.cell[at] = cd.cell;
      ++at;
    }
  }
}

struct IcView {
  int n;
  const PyramidLevelDev* levels; // of every frame of the call, frame after frame
  const int* level_index;        // [n] the keypoint's entry of `levels`
  const float2* xy;              // [n]
  float* angle; int* m10; int* m01;
};

__global__ __launch_bounds__(kIcBlock) void k_ic_angle(IcView v) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * kIcBlock + threadIdx.x;
  if (i >= v.n) return;
  const PyramidLevelDev L = v.levels[v.level_index[i]];
  const float2 p = v.xy[i];
  const unsigned char* center = L.data + (size_t)fast_cv_round(p.y) * L.cols + fast_cv_round(p.x);
  int m10, m01;
  fast_ic_moments(center, (long long)L.cols, m10, m01);
  v.m10[i] = m10; v.m01[i] = m01;
  v.angle[i] = fast_atan2((float)m01, (float)m10);
}

// What a detector frame brings besides its pyramid
static int fast_validate_params(const char* entry, int k, int ini_th, int min_th, const osh_fast_result& r) {
  if (ini_th < 1 || ini_th > 255 || min_th < 1 || min_th > 255) { set_error("%s: frame %d: threshold outside [1, 255]", entry, k); return OSH_ERR_INVALID; }
  if (min_th > ini_th) { set_error("%s: frame %d: min_th %d > ini_th %d", entry, k, min_th, ini_th); return OSH_ERR_INVALID; }
  if (r.capacity < 0 || r.cell_capacity < 0) { set_error("%s: frame %d: negative capacity", entry, k); return OSH_ERR_INVALID; }
  if (!r.level_count) { set_error("%s: frame %d: NULL level_count", entry, k); return OSH_ERR_INVALID; }
  if (r.capacity && (!r.xy || !r.response)) { set_error("%s: frame %d: NULL result array with capacity %d", entry, k, r.capacity); return OSH_ERR_INVALID; }
  return OSH_OK;
}

static int fast_validate(int n_frames, const osh_fast_frame* frames, const osh_fast_result* results) {
  for (int k = 0; k < n_frames; ++k) {
    OSH_TRY(fast_validate_pyramid("osh_orb_fast_detect", k, frames[k].n_levels, frames[k].pyramid));
    OSH_TRY(fast_validate_params("osh_orb_fast_detect", k, frames[k].ini_th, frames[k].min_th, results[k]));
  }
  return OSH_OK;
}

// The cells of a detector call in (frame, level, i, j) order, frame after frame
struct FastPlan {
  std::vector<FastFrameHost> fh;
  std::vector<FastLevelHost> lh;
  std::vector<FastCellDev> cells;
};
// One more level of the plan's last frame: rows x cols pixels at img_off of the resident pyramid
static int fast_plan_level(const char* entry, FastPlan& p, int l, int rows, int cols, long long img_off, int ini_th, int min_th) {
  const int k = (int)p.fh.size() - 1;
  FastLevelHost L{img_off, rows, cols, (int)p.cells.size(), 0};
  const FastGeom g = fast_geometry(rows, cols);
  FastRect r;
  for (int i = 0; i < g.n_rows; ++i)
    for (int j = 0; j < g.n_cols; ++j) {
      if (!fast_cell_rect(g, i, j, r)) continue;
      if (r.w > kFastMaxCell || r.h > kFastMaxCell || r.x0 + r.w > cols || r.y0 + r.h > rows) { set_error("%s: frame %d level %d: cell (%d, %d) out of bounds", entry, k, l, i, j); return OSH_ERR_UNSUPPORTED; }
      p.cells.push_back({L.img_off, cols, r.x0, r.y0, r.w, r.h, j * g.w_cell, i * g.h_cell, l, (int)p.cells.size() - p.fh[k].cell0, ini_th, min_th});
    }
  L.n_cells = (int)p.cells.size() - L.cell0;
  p.lh.push_back(L);
  if (p.cells.size() > (size_t)1 << 22) { set_error("%s: batch too large", entry); return OSH_ERR_UNSUPPORTED; }
  return OSH_OK;
}

// The keypoints of an ic_angle frame against its levels
static int ic_validate_keypoints(int k, const osh_ic_angle_frame& f, int n_levels, const PyramidLevel* lv) {
  if (f.n < 0) { set_error("osh_orb_ic_angle: frame %d: negative keypoint count", k); return OSH_ERR_INVALID; }
  if (f.n && (!f.xy || !f.level)) { set_error("osh_orb_ic_angle: frame %d: NULL keypoint array with n = %d", k, f.n); return OSH_ERR_INVALID; }
  return validate_keypoints("osh_orb_ic_angle", k, f.n, f.xy, f.level, n_levels, lv, kFastHalfPatch, "disc");
}

}  // namespace osh

using namespace osh;

// The kernels of a planned detector call over the resident pyramid and the results of every frame.  `frames` (osh_orb_fast_detect):
// their levels are staged into st->pyramid.h_images and uploaded into its buffer first, img_bytes of them; nullptr: the pyramid is there.
// The caller writes the tokens into the results.
// `frames` (osh_orb_fast_detect) as below.  What it leaves: the candidates on the device in st->emitted, where osh_orb_extract's
// octree reads them, and the offsets and used_min_th on the host in st->call's output.
struct FastEmitRun {
  const int* offset = nullptr;            // host, [n_cells + 1]
  const unsigned char* used = nullptr;    // host, [n_cells]
  size_t total = 0, bytes = 0;            // candidates of the call; bytes of their four arrays
  Section<float2> xy{0}; Section<float> response{0}; Section<int> level{0}, cell{0};   // in st->emitted / st->h_emitted
};
static int fast_emit(const char* entry, FastState* st, hipStream_t s, PhaseClock& clock, const FastPlan& p, const osh_fast_frame* frames, size_t img_bytes,
                     FastEmitRun& run) {
  const int n_cells = (int)p.cells.size(), n_frames = (int)p.fh.size();
  std::vector<int> order(n_cells);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p.cells[a].w * p.cells[a].h > p.cells[b].w * p.cells[b].h; });

  Layout in, out, work;
  const auto s_cells = in.take<FastCellDev>(n_cells);
  const auto s_order = in.take<int>(n_cells);
  const auto o_offset = out.take<int>((size_t)n_cells + 1);
  const auto o_used = out.take<unsigned char>(n_cells);
  const auto w_count = work.take<int>(n_cells);
  const auto w_mask = work.take<unsigned>((size_t)n_cells * kFastMaskWords);
  OSH_TRY(st->call.reserve(in, out, work.bytes));
  char* h = st->call.host_in();
  if (n_cells) {
    std::memcpy(s_cells.in(h), p.cells.data(), sizeof(FastCellDev) * n_cells);
    std::memcpy(s_order.in(h), order.data(), sizeof(int) * n_cells);
  }
  if (frames) {
    OSH_TRY(st->pyramid.buffer.reserve(img_bytes));
    unsigned char* hi = static_cast<unsigned char*>(st->pyramid.h_images.reserve(img_bytes));
    if (!hi) { set_error("%s: pinned allocation of %zu bytes failed", entry, img_bytes); return OSH_ERR_DEVICE; }
    for (int k = 0; k < n_frames; ++k)
      for (int l = 0; l < frames[k].n_levels; ++l) pack_level(hi + p.lh[p.fh[k].level0 + l].img_off, frames[k].pyramid[l]);
  }
  clock.mark();
  OSH_TRY(st->call.upload(s));
  if (frames) OSH_HIP(hipMemcpyAsync(st->pyramid.buffer.p, st->pyramid.h_images.p, img_bytes, hipMemcpyHostToDevice, s));
  OSH_TRY(clock.mark_synced(s));

  FastView v{};
  char* di = st->call.dev_in(); char* dout = st->call.dev_out(); char* dw = st->call.dev_work();
  v.n_cells = n_cells; v.cells = s_cells.in(di); v.order = s_order.in(di); v.images = st->pyramid.images();
  v.mask = w_mask.in(dw); v.count = w_count.in(dw); v.offset = o_offset.in(dout); v.used_min = o_used.in(dout);
  if (n_cells) hipLaunchKernelGGL(k_fast_cells, dim3((unsigned)n_cells), dim3(kFcBlock), 0, s, v);
  hipLaunchKernelGGL(k_fast_scan, dim3(1), dim3(kScanBlock), 0, s, v);
  OSH_TRY(launch_check("FAST cells"));
  OSH_TRY(st->call.download(s));   // offsets and used_min; synchronises
  const int* offset = o_offset.in(st->call.host_out());
  const unsigned char* used = o_used.in(st->call.host_out());
  const size_t total = (size_t)offset[n_cells];

  Layout em;
  const auto e_xy = em.take<float2>(total); const auto e_resp = em.take<float>(total);
  const auto e_level = em.take<int>(total); const auto e_cell = em.take<int>(total);
  if (total) {
    OSH_TRY(st->emitted.reserve(em.bytes));
    char* de = st->emitted.as<char>();
    v.xy = e_xy.in(de); v.response = e_resp.in(de); v.level = e_level.in(de); v.cell = e_cell.in(de);
    hipLaunchKernelGGL(k_fast_emit, dim3((unsigned)n_cells), dim3(64), 0, s, v);
    OSH_TRY(launch_check("FAST emit"));
  }
  run.offset = offset; run.used = used; run.total = total; run.bytes = em.bytes;
  run.xy = e_xy; run.response = e_resp; run.level = e_level; run.cell = e_cell;
  return OSH_OK;
}

// The candidates of a fast_emit down to the host and into the results of every frame
static int fast_download(const char* entry, FastState* st, hipStream_t s, const FastPlan& p, const FastEmitRun& run, osh_fast_result* results) {
  const int n_frames = (int)p.fh.size();
  const int* offset = run.offset;
  const unsigned char* used = run.used;
  const auto e_xy = run.xy; const auto e_resp = run.response; const auto e_level = run.level; const auto e_cell = run.cell;
  if (run.total) {
    if (!st->h_emitted.reserve(run.bytes)) { set_error("%s: pinned allocation of %zu bytes failed", entry, run.bytes); return OSH_ERR_DEVICE; }
    OSH_HIP(hipMemcpyAsync(st->h_emitted.p, st->emitted.p, run.bytes, hipMemcpyDeviceToHost, s));
    OSH_HIP(hipStreamSynchronize(s));
  }
  const char* he = static_cast<const char*>(st->h_emitted.p);
  for (int k = 0; k < n_frames; ++k) {
    osh_fast_result& r = results[k];
    const FastFrameHost& F = p.fh[k];
    const size_t base = (size_t)offset[F.cell0], n = (size_t)offset[F.cell0 + F.n_cells] - base;
    r.n_out = (int32_t)n; r.n_cells = F.n_cells;
    for (int l = 0; l < F.n_levels; ++l) {
      const FastLevelHost& L = p.lh[F.level0 + l];
      r.level_count[l] = offset[L.cell0 + L.n_cells] - offset[L.cell0];
    }
    if (n > (size_t)r.capacity || (r.used_min_th && F.n_cells > r.cell_capacity)) continue;   // counts only: the caller sizes its arrays and calls again
    if (r.used_min_th && F.n_cells) std::memcpy(r.used_min_th, used + F.cell0, (size_t)F.n_cells);
    if (n) {
      scatter(reinterpret_cast<float2*>(r.xy), e_xy, he, base, n); scatter(r.response, e_resp, he, base, n);
      scatter(r.level, e_level, he, base, n); scatter(r.cell, e_cell, he, base, n);
    }
  }
  return OSH_OK;
}

static int fast_run(const char* entry, FastState* st, hipStream_t s, PhaseClock& clock, const FastPlan& p, const osh_fast_frame* frames, size_t img_bytes,
                    osh_fast_result* results) {
  FastEmitRun run;
  OSH_TRY(fast_emit(entry, st, s, clock, p, frames, img_bytes, run));
  OSH_TRY(clock.mark_synced(s));
  return fast_download(entry, st, s, p, run, results);
}

// The plan of a detector call over frames of the resident pyramid; OSH_ERR_INVALID for a token that names none of them
static int fast_plan_resident(const char* entry, const FastState* st, int n_frames, const osh_fast_resident_frame* frames, FastPlan& p) {
  for (int k = 0; k < n_frames; ++k) {
    const FastFrameHost* F = st->pyramid.frame(frames[k].pyramid_token);
    if (!F) { set_error("%s: frame %d: the token names no frame of this context's resident pyramid", entry, k); return OSH_ERR_INVALID; }
    p.fh.push_back({(int)p.lh.size(), F->n_levels, (int)p.cells.size(), 0});
    for (int l = 0; l < F->n_levels; ++l) {
      const FastLevelHost& L = st->pyramid.levels[F->level0 + l];
      OSH_TRY(fast_plan_level(entry, p, l, L.rows, L.cols, L.img_off, frames[k].ini_th, frames[k].min_th));
    }
    p.fh[k].n_cells = (int)p.cells.size() - p.fh[k].cell0;
  }
  return OSH_OK;
}

int osh::fast_emit_resident(const char* entry, osh_orb_ctx* c, hipStream_t s, int n_frames, const osh_fast_resident_frame* frames, FastEmitted& e) {
  FastState* st = orb_state<FastState>(c, kOrbAttachFast);
  FastPlan p;
  OSH_TRY(fast_plan_resident(entry, st, n_frames, frames, p));
  PhaseClock clock;
  FastEmitRun run;
  OSH_TRY(fast_emit(entry, st, s, clock, p, nullptr, 0, run));
  e.levels.clear(); e.level0.clear();
  for (int k = 0; k < n_frames; ++k) {
    e.level0.push_back((int)e.levels.size());
    for (int l = 0; l < p.fh[k].n_levels; ++l) {
      const FastLevelHost& L = p.lh[p.fh[k].level0 + l];
      e.levels.push_back({L.rows, L.cols, L.img_off, run.offset[L.cell0], run.offset[L.cell0 + L.n_cells] - run.offset[L.cell0]});
    }
  }
  e.level0.push_back((int)e.levels.size());
  e.images = st->pyramid.images();
  e.xy = run.total ? run.xy.in(st->emitted.as<const char>()) : nullptr;
  e.response = run.total ? run.response.in(st->emitted.as<const char>()) : nullptr;
  return OSH_OK;
}

int osh::ic_angle_launch(hipStream_t s, int n, const PyramidLevelDev* levels, const int* level_index, const float2* xy, float* angle, int* m10, int* m01) {
  IcView v{};
  v.n = n; v.levels = levels; v.level_index = level_index; v.xy = xy; v.angle = angle; v.m10 = m10; v.m01 = m01;
  hipLaunchKernelGGL(k_ic_angle, dim3((unsigned)((n + kIcBlock - 1) / kIcBlock)), dim3(kIcBlock), 0, s, v);
  return launch_check("IC_Angle");
}

extern "C" int osh_orb_fast_detect(osh_orb_ctx* c, int32_t n_frames, const osh_fast_frame* frames, osh_fast_result* results) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_fast_detect: bad arguments"); return OSH_ERR_INVALID; }
  OSH_TRY(fast_validate(n_frames, frames, results));   // a refusal needs no context and no device
  if (!c) { set_error("osh_orb_fast_detect: no context"); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;

  // the levels packed one after another
  FastPlan p;
  size_t img_bytes = 0;
  for (int k = 0; k < n_frames; ++k) {
    const osh_fast_frame& f = frames[k];
    p.fh.push_back({(int)p.lh.size(), f.n_levels, (int)p.cells.size(), 0});
    for (int l = 0; l < f.n_levels; ++l) {
      OSH_TRY(fast_plan_level("osh_orb_fast_detect", p, l, f.pyramid[l].rows, f.pyramid[l].cols, (long long)img_bytes, f.ini_th, f.min_th));
      img_bytes += (size_t)f.pyramid[l].rows * f.pyramid[l].cols;
      if (img_bytes > (size_t)1 << 31) { set_error("osh_orb_fast_detect: batch too large"); return OSH_ERR_UNSUPPORTED; }
    }
    p.fh[k].n_cells = (int)p.cells.size() - p.fh[k].cell0;
  }

  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  FastState* st = orb_state<FastState>(c, kOrbAttachFast);
  clock.profiling = orb_profiling(c);
  st->pyramid.invalidate();   // the resident pyramid is about to be replaced
  OSH_TRY(fast_run("osh_orb_fast_detect", st, s, clock, p, frames, img_bytes, results));
  const uint64_t token0 = st->pyramid.commit(std::move(p.fh), std::move(p.lh));
  for (int k = 0; k < n_frames; ++k) results[k].pyramid_token = token0 + (uint64_t)k;
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_fast_detect_resident(osh_orb_ctx* c, int32_t n_frames, const osh_fast_resident_frame* frames, osh_fast_result* results) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_fast_detect_resident: bad arguments"); return OSH_ERR_INVALID; }
  for (int k = 0; k < n_frames; ++k) OSH_TRY(fast_validate_params("osh_orb_fast_detect_resident", k, frames[k].ini_th, frames[k].min_th, results[k]));
  if (!c) { set_error("osh_orb_fast_detect_resident: no context"); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  FastState* st = orb_state<FastState>(c, kOrbAttachFast);
  FastPlan p;
  OSH_TRY(fast_plan_resident("osh_orb_fast_detect_resident", st, n_frames, frames, p));
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  clock.profiling = orb_profiling(c);
  OSH_TRY(fast_run("osh_orb_fast_detect_resident", st, s, clock, p, nullptr, 0, results));   // the pyramid and its tokens stay
  for (int k = 0; k < n_frames; ++k) results[k].pyramid_token = frames[k].pyramid_token;
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_ic_angle(osh_orb_ctx* c, int32_t n_frames, const osh_ic_angle_frame* frames, const osh_ic_angle_result* results) {
  PhaseClock clock;
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_ic_angle: bad arguments"); return OSH_ERR_INVALID; }
  PyramidLevels<osh_ic_angle_frame> pl{"osh_orb_ic_angle", n_frames, frames};
  const auto keypoints = [&](int k, int n_levels, const PyramidLevel* lv) { return ic_validate_keypoints(k, frames[k], n_levels, lv); };
  OSH_TRY(pl.check_brought(keypoints));
  if (!c) { set_error("osh_orb_ic_angle: no context"); return OSH_ERR_INVALID; }
  FastState* st = pl.any_token ? orb_state<FastState>(c, kOrbAttachFast) : nullptr;
  OSH_TRY(pl.check_tokens(st ? &st->pyramid : nullptr, keypoints));
  size_t N = 0;
  for (int k = 0; k < n_frames; ++k) N += (size_t)frames[k].n;
  if (N > (size_t)1 << 24) { set_error("osh_orb_ic_angle: more than 2^24 keypoints in one call"); return OSH_ERR_UNSUPPORTED; }
  if (N == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  if (!st) st = orb_state<FastState>(c, kOrbAttachFast);
  clock.profiling = orb_profiling(c);

  OSH_TRY(pl.list(&st->pyramid));
  Layout in, out;
  const auto s_levels = in.take<PyramidLevelDev>(pl.lv.size());
  const auto s_index = in.take<int>(N);
  const auto s_xy = in.take<float2>(N);
  const auto s_img = in.take<unsigned char>(pl.img_bytes);
  const auto o_angle = out.take<float>(N); const auto o_m10 = out.take<int>(N); const auto o_m01 = out.take<int>(N);
  OSH_TRY(st->ic_call.reserve(in, out));
  char* h = st->ic_call.host_in();
  const unsigned char* uploaded = s_img.in(static_cast<const char*>(st->ic_call.dev_in()));
  for (size_t l = 0; l < pl.lv.size(); ++l) s_levels.in(h)[l] = {pl.data(l, st->pyramid.images(), uploaded), pl.lv[l].rows, pl.lv[l].cols};
  pl.index(s_index.in(h));
  pl.stage(s_img.in(h));
  std::vector<size_t> base(n_frames);
  size_t b = 0;
  for (int k = 0; k < n_frames; ++k) {
    base[k] = b;
    if (frames[k].n) std::memcpy(s_xy.in(h) + b, frames[k].xy, (size_t)frames[k].n * 8);
    b += (size_t)frames[k].n;
  }
  clock.mark();
  OSH_TRY(st->ic_call.upload(s));
  OSH_TRY(clock.mark_synced(s));
  char* di = st->ic_call.dev_in(); char* dout = st->ic_call.dev_out();
  OSH_TRY(ic_angle_launch(s, (int)N, s_levels.in(di), s_index.in(di), s_xy.in(di), o_angle.in(dout), o_m10.in(dout), o_m01.in(dout)));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->ic_call.download(s));
  const char* ho = st->ic_call.host_out();
  for (int k = 0; k < n_frames; ++k) {
    const size_t n = (size_t)frames[k].n;
    scatter(results[k].angle, o_angle, ho, base[k], n); scatter(results[k].m10, o_m10, ho, base[k], n); scatter(results[k].m01, o_m01, ho, base[k], n);
  }
  clock.mark();
  clock.store(st->ms_ic);
  return OSH_OK;
}

extern "C" int osh_orb_fast_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<FastState>("osh_orb_fast_get_times", c, kOrbAttachFast, ms);
}

extern "C" int osh_orb_ic_angle_get_times(osh_orb_ctx* c, double ms[4]) {
  if (!c || !ms) { set_error("osh_orb_ic_angle_get_times: bad arguments"); return OSH_ERR_INVALID; }
  std::memcpy(ms, orb_state<FastState>(c, kOrbAttachFast)->ms_ic, sizeof(double) * 4);
  return OSH_OK;
}
