// orb_fuse_device.hip -- the search of ORBmatcher::Fuse (src/ORBmatcher.cc:1148-1455) for one map point list and MANY target
// keyframes in one call on MI355X (gfx950); the statements are those of orb_fuse.h.
//
// Two kernels with a compaction between them.  The geometry of a pair is a few dozen float operations with no memory traffic to
// speak of, and most pairs end in it (a neighbour keyframe sees a minority of the list): k_fuse_project runs it with one THREAD per
// pair, all lanes busy, writes every output word of the pair and appends the survivors to a list (one atomic per wavefront: ballot,
// one add by the first surviving lane, ranks from the ballot).  The search of a survivor walks a handful of grid cells and compares
// 32-byte descriptors: k_fuse_search gives it one WAVEFRONT, lane c walking cell c of the window as k_orb_grid does, over a grid
// sized by the device and not by the pair count (the wavefronts stride the list, whose length only the device knows).  One fused
// kernel with an early exit would either spend a wavefront on every rejected pair or leave the search to single lanes; a
// prefix-sum compaction would add a third launch for an order nothing depends on.
// The list order differs from run to run; no result does: a pair's words are written by its own thread, then by lane 0 of its own
// wavefront, and depend on nothing but the pair.
// Candidate key = (distance << 22) | (cell of the window << 8) | entry in the cell: the minimum is the first least candidate of the
// reference's scan (ix-major, iy, insertion order).  14 bits of cell cover OSH_FUSE_MAX_CELLS, 8 bits of entry
// OSH_FUSE_MAX_CELL_ENTRIES.
#include "common.h"
#include "orb_fuse.h"
#include "orb_grid_bin.h"
#include "orb_hamming.h"
#include "orb_stage.h"
#include <cmath>
#include <vector>

namespace osh {

constexpr int kFuseBlock = 256;
constexpr int kFuseWaves = kFuseBlock / 64;
constexpr int kFuseSearchBlocks = 2048;   // 256 CUs x 8 blocks of four wavefronts
static_assert(OSH_FUSE_MAX_CELLS <= (1 << 14) && OSH_FUSE_MAX_CELL_ENTRIES < (1 << 8) && kPosBits == 22, "the position key is 14 + 8 bits");

struct FuseView {
  int K, P, mode;
  const FuseTarget* target;                    // [K]
  const int* cell_off; const int* cell_idx;    // concatenated: FuseTarget::cell_base / key_base
  const float* key_xy; const int* key_octave; const float* key_uright; const uint4* key_desc;
  const float* pos; const float* normal; const float* min_dist; const float* max_dist; const unsigned char* skip; const uint4* pdesc;
  int* stage; float* u; float* v; float* ur; int* level; float* radius; int* n_candidates; int* best_idx; int* best_dist;   // [K*P]
  int* list; int* n_listed;
};

// grid = (ceil(P / 256), K)
__global__ __launch_bounds__(kFuseBlock) void k_fuse_project(FuseView w) {
  const int t = (int)blockIdx.y;
  const int p = (int)blockIdx.x * kFuseBlock + (int)threadIdx.x;
  const int lane = (int)(threadIdx.x & 63);
  const bool valid = p < w.P;
  const int pp = valid ? p : 0;
  const FuseTarget& T = w.target[t];
  const float P3[3] = {w.pos[3 * pp], w.pos[3 * pp + 1], w.pos[3 * pp + 2]};
  const float Pn[3] = {w.normal[3 * pp], w.normal[3 * pp + 1], w.normal[3 * pp + 2]};
  FuseGeom g;
  fuse_project(T, P3, Pn, w.min_dist[pp], w.max_dist[pp], w.skip[pp] != 0, g);
  const int pair = t * w.P + pp;
  const bool live = valid && g.stage == OSH_FUSE_SEARCHED;
  if (valid) {
    w.stage[pair] = g.stage; w.u[pair] = g.u; w.v[pair] = g.v; w.ur[pair] = g.ur; w.level[pair] = g.level; w.radius[pair] = g.radius;
    w.n_candidates[pair] = 0; w.best_idx[pair] = -1; w.best_dist[pair] = 256;
  }
  const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
  if (m) {
    const int leader = __builtin_ctzll(m);
    int base = 0;
    if (lane == leader) base = atomicAdd(w.n_listed, __popcll(m));
    base = __shfl(base, leader, 64);
    if (live) w.list[base + __popcll(m & ((1ull << lane) - 1ull))] = pair;
  }
}

// grid = min(ceil(K * P / 4), kFuseSearchBlocks): the wavefronts stride the list
__global__ __launch_bounds__(kFuseBlock) void k_fuse_search(FuseView w) {
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kFuseWaves + (int)(threadIdx.x >> 6));
  const int n_waves = (int)gridDim.x * kFuseWaves;
  const int count = *w.n_listed;
  for (int s = wave; s < count; s += n_waves) {
    const int pair = __builtin_amdgcn_readfirstlane(w.list[s]);
    const int t = pair / w.P, p = pair - t * w.P;
    const FuseTarget& T = w.target[t];
    FuseGeom g;
    g.stage = OSH_FUSE_SEARCHED; g.u = w.u[pair]; g.v = w.v[pair]; g.ur = w.ur[pair]; g.level = w.level[pair]; g.radius = w.radius[pair];
    const FuseWindow win = fuse_window(T, g.u, g.v, g.radius);
    FuseKeys keys;
    keys.xy = w.key_xy + 2 * (size_t)T.key_base; keys.octave = w.key_octave + T.key_base; keys.uright = w.key_uright + T.key_base;
    keys.desc = nullptr; keys.cell_off = w.cell_off + T.cell_base; keys.cell_idx = w.cell_idx + T.key_base;
    const uint4* kd = w.key_desc + 2 * (size_t)T.key_base;
    const uint4 a0 = w.pdesc[2 * (size_t)p], a1 = w.pdesc[2 * (size_t)p + 1];
    const int ncell = win.nx * win.ny;
    unsigned best = 0xFFFFFFFFu;
    int n_in = 0, n_cand = 0;
    for (int c = lane; c < ncell; c += 64) {
      const int cx = c / win.ny, cy = c - cx * win.ny;
      const int cell = (win.x0 + cx) * T.rows + (win.y0 + cy);
      const int k0 = keys.cell_off[cell], k1 = keys.cell_off[cell + 1];
      for (int k = k0; k < k1; ++k) {
        const int idx = keys.cell_idx[k];
        const int kind = fuse_candidate(T, keys, idx, g, w.mode);
        if (kind == 0) continue;
        ++n_in;
        if (kind == 1) continue;
        ++n_cand;
        const unsigned d = hamming256(a0, a1, kd[2 * (size_t)idx], kd[2 * (size_t)idx + 1]);
        best = min(best, (d << kPosBits) | ((unsigned)c << 8) | (unsigned)(k - k0));
      }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      best = min(best, (unsigned)__shfl_xor((int)best, m, 64));
      n_in += __shfl_xor(n_in, m, 64);
      n_cand += __shfl_xor(n_cand, m, 64);
    }
    if (lane == 0) {
      if (n_in == 0) w.stage[pair] = OSH_FUSE_EMPTY;
      w.n_candidates[pair] = n_cand;
      const unsigned bd = best >> kPosBits;
      if (best != 0xFFFFFFFFu && bd < 256u) {   // a candidate at distance 256 never wins: bestDist starts at 256
        const unsigned pos = best & kPosMask;
        const int c = (int)(pos >> 8), k = (int)(pos & 0xffu);
        const int cx = c / win.ny, cy = c - cx * win.ny;
        w.best_idx[pair] = keys.cell_idx[keys.cell_off[(win.x0 + cx) * T.rows + (win.y0 + cy)] + k];
        w.best_dist[pair] = (int)bd;
      }
    }
  }
}

struct FuseState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

static bool finite_all(const float* a, int n) {
  for (int k = 0; k < n; ++k) if (!std::isfinite(a[k])) return false;
  return true;
}

// Everything a refusal rests on: needs no context and no device
static int fuse_validate(int n_targets, const osh_fuse_target* targets, const osh_fuse_points* points, int mode, const osh_fuse_result* result,
                         size_t* total_keys, size_t* total_cells) {
  if (n_targets < 0) { set_error("osh_orb_fuse_search: n_targets %d is negative", n_targets); return OSH_ERR_INVALID; }
  if (!points) { set_error("osh_orb_fuse_search: points is NULL"); return OSH_ERR_INVALID; }
  if (points->n < 0) { set_error("osh_orb_fuse_search: points: n %d is negative", points->n); return OSH_ERR_INVALID; }
  if (n_targets && !targets) { set_error("osh_orb_fuse_search: targets is NULL with n_targets = %d", n_targets); return OSH_ERR_INVALID; }
  if (mode != OSH_FUSE_CHI2 && mode != OSH_FUSE_SIM3) { set_error("osh_orb_fuse_search: unknown mode %d", mode); return OSH_ERR_INVALID; }
  if (points->n) {
    const struct { const void* p; const char* name; } arrays[] = {{points->pos, "pos"}, {points->normal, "normal"}, {points->min_dist, "min_dist"},
                                                                  {points->max_dist, "max_dist"}, {points->desc, "desc"}};
    for (const auto& a : arrays)
      if (!a.p) { set_error("osh_orb_fuse_search: points: %s is NULL with n = %d", a.name, points->n); return OSH_ERR_INVALID; }
  }
  if (n_targets && points->n && !result) { set_error("osh_orb_fuse_search: result is NULL"); return OSH_ERR_INVALID; }
  if (n_targets > OSH_FUSE_MAX_TARGETS) { set_error("osh_orb_fuse_search: %d targets, more than OSH_FUSE_MAX_TARGETS = %d", n_targets, OSH_FUSE_MAX_TARGETS); return OSH_ERR_UNSUPPORTED; }
  if (points->n > OSH_FUSE_MAX_POINTS) { set_error("osh_orb_fuse_search: %d points, more than OSH_FUSE_MAX_POINTS = %d", points->n, OSH_FUSE_MAX_POINTS); return OSH_ERR_UNSUPPORTED; }
  if ((long long)n_targets * points->n > (1ll << 27)) { set_error("osh_orb_fuse_search: %d x %d pairs, more than 2^27", n_targets, points->n); return OSH_ERR_UNSUPPORTED; }
  size_t keys = 0, cells = 0;
  for (int t = 0; t < n_targets; ++t) {
    const osh_fuse_target& T = targets[t];
    if (!finite_all(T.Rcw, 9) || !finite_all(T.tcw, 3) || !finite_all(T.Ow, 3)) { set_error("target %d: pose (Rcw, tcw, Ow) is not finite", t); return OSH_ERR_INVALID; }
    if (T.camera != OSH_FUSE_PINHOLE && T.camera != OSH_FUSE_KB8) { set_error("target %d: unknown camera kind %d", t, T.camera); return OSH_ERR_INVALID; }
    const float cam[5] = {T.fx, T.fy, T.cx, T.cy, T.bf};
    if (!finite_all(cam, 5) || (T.camera == OSH_FUSE_KB8 && !finite_all(T.kb8, 4))) { set_error("target %d: camera (fx, fy, cx, cy, kb8, bf) is not finite", t); return OSH_ERR_INVALID; }
    const float bounds[4] = {T.min_x, T.max_x, T.min_y, T.max_y};
    if (!finite_all(bounds, 4)) { set_error("target %d: image bounds are not finite", t); return OSH_ERR_INVALID; }
    if (!std::isfinite(T.th)) { set_error("target %d: th is not finite", t); return OSH_ERR_INVALID; }
    if (T.n_levels < 1 || T.n_levels > OSH_FUSE_MAX_LEVELS) { set_error("target %d: n_levels %d outside [1, %d]", t, T.n_levels, OSH_FUSE_MAX_LEVELS); return OSH_ERR_INVALID; }
    if (!std::isfinite(T.log_scale_factor) || !finite_all(T.scale_factors, T.n_levels) || !finite_all(T.inv_level_sigma2, T.n_levels)) {
      set_error("target %d: level tables (log_scale_factor, scale_factors, inv_level_sigma2) are not finite", t); return OSH_ERR_INVALID;
    }
    if (T.cols <= 0 || T.rows <= 0) { set_error("target %d: grid size %d x %d is not positive", t, T.cols, T.rows); return OSH_ERR_INVALID; }
    if (!(T.cell_w_inv > 0.f) || !(T.cell_h_inv > 0.f) || !std::isfinite(T.cell_w_inv) || !std::isfinite(T.cell_h_inv)) {
      set_error("target %d: cell inverse (cell_w_inv, cell_h_inv) is not positive and finite", t); return OSH_ERR_INVALID;
    }
    if (!std::isfinite(T.grid_min_x) || !std::isfinite(T.grid_min_y)) { set_error("target %d: grid origin (grid_min_x, grid_min_y) is not finite", t); return OSH_ERR_INVALID; }
    if (T.n_keys < 0) { set_error("target %d: n_keys %d is negative", t, T.n_keys); return OSH_ERR_INVALID; }
    if (T.n_keys && (!T.key_xy || !T.key_octave || !T.descriptors)) { set_error("target %d: NULL keypoint array (key_xy, key_octave, descriptors) with n_keys = %d", t, T.n_keys); return OSH_ERR_INVALID; }
    if ((long long)T.cols * T.rows > OSH_FUSE_MAX_CELLS) { set_error("target %d: %d x %d grid cells, more than OSH_FUSE_MAX_CELLS = %d", t, T.cols, T.rows, OSH_FUSE_MAX_CELLS); return OSH_ERR_UNSUPPORTED; }
    if (T.n_keys > OSH_FUSE_MAX_KEYS) { set_error("target %d: n_keys %d, more than OSH_FUSE_MAX_KEYS = %d", t, T.n_keys, OSH_FUSE_MAX_KEYS); return OSH_ERR_UNSUPPORTED; }
    for (int i = 0; i < T.n_keys; ++i) {
      if (T.key_octave[i] < 0 || T.key_octave[i] >= T.n_levels) { set_error("target %d: keypoint %d: key_octave %d outside [0, %d)", t, i, T.key_octave[i], T.n_levels); return OSH_ERR_INVALID; }
      if (!std::isfinite(T.key_xy[2 * i]) || !std::isfinite(T.key_xy[2 * i + 1])) { set_error("target %d: keypoint %d: key_xy is not finite", t, i); return OSH_ERR_INVALID; }
    }
    keys += (size_t)T.n_keys; cells += (size_t)T.cols * T.rows + 1;
  }
  *total_keys = keys; *total_cells = cells;
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

extern "C" int osh_orb_fuse_search(osh_orb_ctx* c, int32_t n_targets, const osh_fuse_target* targets, const osh_fuse_points* points, int32_t mode,
                                   const osh_fuse_result* result) {
  PhaseClock clock;
  size_t NK = 0, NC = 0;
  OSH_TRY(fuse_validate(n_targets, targets, points, mode, result, &NK, &NC));
  const size_t K = (size_t)n_targets, P = (size_t)points->n, KP = K * P;
  Layout in, out;
  const auto s_target = in.take<FuseTarget>(K);
  const auto s_coff = in.take<int>(NC); const auto s_cidx = in.take<int>(NK);
  const auto s_kxy = in.take<float>(NK * 2); const auto s_koct = in.take<int>(NK); const auto s_kur = in.take<float>(NK); const auto s_kdesc = in.take<uint4>(NK * 2);
  const auto s_pos = in.take<float>(P * 3); const auto s_normal = in.take<float>(P * 3); const auto s_mind = in.take<float>(P); const auto s_maxd = in.take<float>(P);
  const auto s_skip = in.take<unsigned char>(P); const auto s_pdesc = in.take<uint4>(P * 2);
  const auto s_count = in.take<int>(1);   // the list's counter, zeroed by the upload
  const auto o_stage = out.take<int>(KP); const auto o_u = out.take<float>(KP); const auto o_v = out.take<float>(KP); const auto o_ur = out.take<float>(KP);
  const auto o_level = out.take<int>(KP); const auto o_radius = out.take<float>(KP); const auto o_ncand = out.take<int>(KP);
  const auto o_bidx = out.take<int>(KP); const auto o_bdist = out.take<int>(KP);

  // the grids are binned before there is a context: a cell above the limit is a refusal
  std::vector<int> coff(NC, 0), cidx(std::max<size_t>(NK, 1), 0), cell_of, fill;
  std::vector<FuseTarget> packed(K);
  size_t kb = 0, cb = 0;
  for (size_t t = 0; t < K; ++t) {
    const osh_fuse_target& T = targets[t];
    fuse_fill_target(T, packed[t]);
    packed[t].key_base = (int)kb; packed[t].cell_base = (int)cb;
    const int most = bin_keypoints(T.key_xy, T.n_keys, T.grid_min_x, T.grid_min_y, T.cell_w_inv, T.cell_h_inv, T.cols, T.rows, OSH_FUSE_MAX_CELL_ENTRIES,
                                   coff.data() + cb, cidx.data() + kb, cell_of, fill);
    if (most > OSH_FUSE_MAX_CELL_ENTRIES) {
      set_error("target %zu: %d keypoints in one grid cell, more than OSH_FUSE_MAX_CELL_ENTRIES = %d", t, most, OSH_FUSE_MAX_CELL_ENTRIES);
      return OSH_ERR_UNSUPPORTED;
    }
    kb += (size_t)T.n_keys; cb += (size_t)T.cols * T.rows + 1;
  }
  if (!c) { set_error("osh_orb_fuse_search: no context"); return OSH_ERR_INVALID; }
  if (KP == 0) return OSH_OK;
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  FuseState* st = orb_state<FuseState>(c, kOrbAttachFuse);
  clock.profiling = orb_profiling(c);
  OSH_TRY(st->call.reserve(in, out, KP * sizeof(int)));

  char* h = st->call.host_in();
  std::memcpy(s_target.in(h), packed.data(), K * sizeof(FuseTarget));
  std::memcpy(s_coff.in(h), coff.data(), NC * sizeof(int));
  if (NK) std::memcpy(s_cidx.in(h), cidx.data(), NK * sizeof(int));
  for (size_t t = 0; t < K; ++t) {
    const osh_fuse_target& T = targets[t];
    const size_t n = (size_t)T.n_keys, b = (size_t)packed[t].key_base;
    if (!n) continue;
    std::memcpy(s_kxy.in(h) + 2 * b, T.key_xy, n * 8); std::memcpy(s_koct.in(h) + b, T.key_octave, n * 4);
    if (T.key_uright) std::memcpy(s_kur.in(h) + b, T.key_uright, n * 4); else std::memset(s_kur.in(h) + b, 0, n * 4);
    std::memcpy(s_kdesc.in(h) + 2 * b, T.descriptors, n * 32);
  }
  std::memcpy(s_pos.in(h), points->pos, P * 12); std::memcpy(s_normal.in(h), points->normal, P * 12);
  std::memcpy(s_mind.in(h), points->min_dist, P * 4); std::memcpy(s_maxd.in(h), points->max_dist, P * 4);
  if (points->skip) std::memcpy(s_skip.in(h), points->skip, P); else std::memset(s_skip.in(h), 0, P);
  std::memcpy(s_pdesc.in(h), points->desc, P * 32);
  *s_count.in(h) = 0;
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  char* di = st->call.dev_in();
  char* dout = st->call.dev_out();
  FuseView v{};
  v.K = (int)K; v.P = (int)P; v.mode = mode;
  v.target = s_target.in(di); v.cell_off = s_coff.in(di); v.cell_idx = s_cidx.in(di);
  v.key_xy = s_kxy.in(di); v.key_octave = s_koct.in(di); v.key_uright = s_kur.in(di); v.key_desc = s_kdesc.in(di);
  v.pos = s_pos.in(di); v.normal = s_normal.in(di); v.min_dist = s_mind.in(di); v.max_dist = s_maxd.in(di); v.skip = s_skip.in(di); v.pdesc = s_pdesc.in(di);
  v.stage = o_stage.in(dout); v.u = o_u.in(dout); v.v = o_v.in(dout); v.ur = o_ur.in(dout); v.level = o_level.in(dout); v.radius = o_radius.in(dout);
  v.n_candidates = o_ncand.in(dout); v.best_idx = o_bidx.in(dout); v.best_dist = o_bdist.in(dout);
  v.list = reinterpret_cast<int*>(st->call.dev_work()); v.n_listed = s_count.in(di);
  hipLaunchKernelGGL(k_fuse_project, dim3((unsigned)((P + kFuseBlock - 1) / kFuseBlock), (unsigned)K), dim3(kFuseBlock), 0, s, v);
  OSH_TRY(launch_check("fuse search (projection)"));
  const size_t blocks = std::min<size_t>((KP + kFuseWaves - 1) / kFuseWaves, kFuseSearchBlocks);
  hipLaunchKernelGGL(k_fuse_search, dim3((unsigned)blocks), dim3(kFuseBlock), 0, s, v);
  OSH_TRY(launch_check("fuse search (candidates)"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));
  const char* ho = st->call.host_out();
  scatter(result->stage, o_stage, ho, 0, KP); scatter(result->u, o_u, ho, 0, KP); scatter(result->v, o_v, ho, 0, KP); scatter(result->ur, o_ur, ho, 0, KP);
  scatter(result->level, o_level, ho, 0, KP); scatter(result->radius, o_radius, ho, 0, KP); scatter(result->n_candidates, o_ncand, ho, 0, KP);
  scatter(result->best_idx, o_bidx, ho, 0, KP); scatter(result->best_dist, o_bdist, ho, 0, KP);
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_fuse_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<FuseState>("osh_orb_fuse_get_times", c, kOrbAttachFuse, ms);
}
