// schur_plan_check.cpp -- host-only self check of the Schur work plan (schur_plan.h).
// Builds the plan of one window exactly as osh_lba_upload does and verifies that every pair of
// optimisable observers of every landmark is covered by exactly one item record, that every
// contribution slot is written by exactly one (item, pose pair) and lies in the range of its block
// of S, and that every landmark has exactly one dinv owner.  Needs no GPU.
#include "common.h"
#include "lba_pack.h"
#include "schur_plan.h"
#include <map>
#include <set>

using namespace osh;

// the plan of one window as osh_lba_upload builds it, items of at most item_max landmarks
struct WindowPlan {
  std::vector<std::vector<int>> obs;   // optimisable-pose edges of every landmark, poses ascending (what upload's sort produces)
  std::vector<int> lmo, nfree, epose;
  SchurPlan plan;
};
static int build_window_plan(const osh_lba_problem* p, int item_max, WindowPlan& wp) {
  const int P = p->n_free, L = p->n_points;
  std::vector<std::vector<int>>& obs = wp.obs;
  std::vector<int>&lmo = wp.lmo, &nfree = wp.nfree, &epose = wp.epose;
  obs.assign(L, {});
  for (int e = 0; e < p->n_edges; ++e) {
    const int ip = p->edge_pose[e], il = p->edge_point[e];
    if (ip < 0 || ip >= P + p->n_fixed || il < 0 || il >= L) { set_error("edge %d out of range", e); return OSH_ERR_INVALID; }
    if (ip < P) obs[il].push_back(ip);
  }
  lmo.assign(L + 1, 0); nfree.assign(L, 0);
  for (int j = 0; j < L; ++j) {
    std::sort(obs[j].begin(), obs[j].end());
    for (size_t k = 1; k < obs[j].size(); ++k)
      if (obs[j][k] == obs[j][k - 1]) { set_error("landmark %d observed twice by pose %d", j, obs[j][k]); return OSH_ERR_UNSUPPORTED; }
    nfree[j] = (int)obs[j].size();
    lmo[j] = (int)epose.size();
    epose.insert(epose.end(), obs[j].begin(), obs[j].end());
  }
  lmo[L] = (int)epose.size();
  epose.push_back(0);
  std::vector<plan_detail::Build> builds;
  std::vector<SRec> brecs;
  plan_detail::PlanScratch psc;
  if (!plan_window(0, P, L, lmo.data(), nfree.data(), epose.data(), builds, brecs, wp.plan, psc, item_max)) { set_error("landmark with > 254 observers"); return OSH_ERR_UNSUPPORTED; }
  std::vector<int> build_win(builds.size(), 0);
  finish_plan(build_win, builds, brecs, wp.plan);
  return OSH_OK;
}

// Shapes of the plan of one window (needs no GPU): hist[sym][nx][ny][landmarks] = items of that shape ([2][9][9][kItemMaxLm + 1]), and the
// matrix-pipe cycles of one pass with whole tiles and with the four-block instructions of the symmetric items, at the 64 and 17
// cycles per instruction that profiles/ubench/mfma_f64_blocks.hip measured.  item_max <= 0: what a call with one window uses.
extern "C" int osh_lba_schur_plan_shapes(const osh_lba_problem* p, int item_max, int64_t* hist, int64_t cycles[2]) {
  if (!p || !hist || !cycles) { set_error("osh_lba_schur_plan_shapes: NULL argument"); return OSH_ERR_INVALID; }
  if (item_max > kItemMaxLm) { set_error("osh_lba_schur_plan_shapes: item_max %d > %d", item_max, kItemMaxLm); return OSH_ERR_INVALID; }
  WindowPlan wp;
  if (const int rc = build_window_plan(p, item_max > 0 ? item_max : item_max_lm(1), wp)) return rc;
  std::fill(hist, hist + 2 * 9 * 9 * (kItemMaxLm + 1), (int64_t)0);
  cycles[0] = cycles[1] = 0;
  for (const SItem& I : wp.plan.items) {
    const int nx = I.shape & 0xff, ny = (I.shape >> 8) & 0xff, sym = (I.shape >> 16) & 1;
    if (nx > 8 || ny > 8 || I.n_lm > kItemMaxLm) { set_error("plan: item of shape (%d, %d), %d landmarks", nx, ny, I.n_lm); return OSH_ERR_DEVICE; }
    hist[((sym * 9 + nx) * 9 + ny) * (kItemMaxLm + 1) + I.n_lm]++;
    const long long ksteps = 6 * (long long)((I.n_lm + 7) / 8);
    const SchurStep t = schur_step(sym, nx, ny, false), b = schur_step(sym, nx, ny, true);
    cycles[0] += ksteps * (64 * t.tiles + 17 * t.blocks);
    cycles[1] += ksteps * (64 * b.tiles + 17 * b.blocks);
  }
  return OSH_OK;
}

// The matrix instructions of one k step of an item of shape (sym, nx, ny) as k_schur_fused issues and stores them (needs no GPU):
// 16 ints per instruction, at most 24 instructions; *n_instr = their number.  {kind, ti, tj, 0, then per block q = 0 .. 3:
// block row, block column, use}.  kind 0: one 16x16x4 of tile (ti, tj), every entry stored where it lies if its pose pair is live.
// kind 1: four blocks of 4 x 4 (block row / column: image rows 4 b .. 4 b + 3); use 0: not stored, 1: stored where it lies, 2: stored
// where it lies and, inside a diagonal pose pair, at the mirrored place too.
extern "C" int osh_lba_schur_block_list(int sym, int nx, int ny, int use_blocks, int32_t* out, int* n_instr) {
  if (!out || !n_instr || nx < 1 || nx > 8 || ny < 1 || ny > 8 || (sym && nx != ny)) { set_error("osh_lba_schur_block_list: invalid argument"); return OSH_ERR_INVALID; }
  SchurInstr list[kSchurInstrMax];
  const int n = schur_instr_list(sym != 0, nx, ny, use_blocks != 0, list);
  for (int k = 0; k < n; ++k) {
    int32_t* o = out + 16 * k;
    o[0] = list[k].kind; o[1] = list[k].ti; o[2] = list[k].tj; o[3] = 0;
    for (int q = 0; q < 4; ++q) { o[4 + 3 * q] = list[k].brow[q]; o[5 + 3 * q] = list[k].bcol[q]; o[6 + 3 * q] = list[k].use[q]; }
  }
  *n_instr = n;
  return OSH_OK;
}

// item_max > 0: the plan cut at that many landmarks per item (8 .. kItemMaxLm: the plan of any size class, checked without the
// environment); <= 0: what a call with one window uses, item_max_lm(1), which OSH_LBA_ITEM_MAX overrides.
extern "C" int osh_lba_schur_plan_stats_cut(const osh_lba_problem* p, int item_max, int64_t stats[8]) {
  if (!p || !stats) { set_error("osh_lba_schur_plan_stats: NULL argument"); return OSH_ERR_INVALID; }
  if (item_max > 0 && (item_max < 8 || item_max > kItemMaxLm)) { set_error("osh_lba_schur_plan_stats_cut: item_max %d outside 8..%d", item_max, kItemMaxLm); return OSH_ERR_INVALID; }
  const int P = p->n_free, L = p->n_points;
  WindowPlan wp;
  if (const int rc = build_window_plan(p, item_max > 0 ? item_max : item_max_lm(1), wp)) return rc;
  const std::vector<std::vector<int>>& obs = wp.obs;
  const std::vector<int>&lmo = wp.lmo, &nfree = wp.nfree;
  const SchurPlan& plan = wp.plan;

  // ---- verification
  std::map<std::pair<int, int>, std::pair<int, int>> range;   // block -> [start, start+count)
  std::vector<std::pair<int, int>> crange(P);
  for (const RBlk& rb : plan.rblk) {
    const int i = rb.ij & 0xffff, j = (rb.ij >> 16) & 0xffff;
    if (j == 0xffff) crange[i] = {rb.start, rb.start + rb.count};
    else range[{i, j}] = {rb.start, rb.start + rb.count};
  }
  if ((int)range.size() != P * (P + 1) / 2) { set_error("plan: %zu blocks of S, expected %d", range.size(), P * (P + 1) / 2); return OSH_ERR_DEVICE; }
  std::vector<int> used(plan.n_contrib, 0), cused(plan.n_ccontrib, 0), owner(L, 0);
  std::vector<std::set<std::pair<int, int>>> covered(L);
  std::vector<std::set<int>> ccovered(L);
  for (size_t it = 0; it < plan.items.size(); ++it) {
    const SItem& I = plan.items[it];
    const bool sym = (I.shape >> 16) & 1;
    if (sym != (it < (size_t)plan.n_sym)) { set_error("plan: item %zu on the wrong side of n_sym", it); return OSH_ERR_DEVICE; }
    const int* X = &plan.pose_x[it * 8];
    const int* Y = &plan.pose_y[it * 8];
    std::set<std::pair<int, int>> live;
    std::set<int> clive;
    for (int r = 0; r < I.n_lm; ++r) {
      const SRec& R = plan.recs[(size_t)I.rec_off + r];
      const unsigned long long xs = R.x_lo | ((unsigned long long)R.x_hi << 32), ys = R.y_lo | ((unsigned long long)R.y_hi << 32);
      if (R.flags & 1) owner[R.lm]++;
      if (R.e_first != lmo[R.lm]) { set_error("plan: record of landmark %d has a wrong first edge", R.lm); return OSH_ERR_DEVICE; }
      for (int sa = 0; sa < 8; ++sa) {
        const unsigned ra = (unsigned)(xs >> (8 * sa)) & 0xff;
        if (ra == kAbsent) continue;
        if ((int)ra >= nfree[R.lm] || obs[R.lm][ra] != X[sa]) { set_error("plan: item %zu slot %d does not match landmark %d", it, sa, R.lm); return OSH_ERR_DEVICE; }
        if (sym) { if (!ccovered[R.lm].insert((int)ra).second) { set_error("plan: rhs term of landmark %d rank %u twice", R.lm, ra); return OSH_ERR_DEVICE; } clive.insert(sa); }
        for (int sb = sym ? sa : 0; sb < 8; ++sb) {
          const unsigned rb = (unsigned)(ys >> (8 * sb)) & 0xff;
          if (rb == kAbsent) continue;
          if ((int)rb >= nfree[R.lm] || obs[R.lm][rb] != Y[sb] || rb < ra) { set_error("plan: item %zu column slot %d does not match landmark %d", it, sb, R.lm); return OSH_ERR_DEVICE; }
          if (!covered[R.lm].insert({(int)ra, (int)rb}).second) { set_error("plan: pair (%u,%u) of landmark %d covered twice", ra, rb, R.lm); return OSH_ERR_DEVICE; }
          live.insert({sa, sb});
        }
      }
    }
    for (int sa = 0; sa < 8; ++sa) {
      const int cs = plan.c_slot[it * 8 + sa];
      if ((cs >= 0) != (clive.count(sa) > 0)) { set_error("plan: item %zu rhs slot %d liveness mismatch", it, sa); return OSH_ERR_DEVICE; }
      if (cs >= 0) {
        if (cs < crange[X[sa]].first || cs >= crange[X[sa]].second) { set_error("plan: rhs slot outside its pose range"); return OSH_ERR_DEVICE; }
        cused[cs]++;
      }
      for (int sb = 0; sb < 8; ++sb) {
        const int ps = plan.pair_slot[it * 64 + sa * 8 + sb];
        if ((ps >= 0) != (live.count({sa, sb}) > 0)) { set_error("plan: item %zu pair (%d,%d) liveness mismatch", it, sa, sb); return OSH_ERR_DEVICE; }
        if (ps >= 0) {
          const auto rg = range.find({X[sa], Y[sb]});
          if (rg == range.end() || ps < rg->second.first || ps >= rg->second.second) { set_error("plan: contribution slot outside its block range"); return OSH_ERR_DEVICE; }
          used[ps]++;
        }
      }
    }
  }
  for (int j = 0; j < L; ++j) {
    const long long k = nfree[j];
    if ((long long)covered[j].size() != k * (k + 1) / 2 || (long long)ccovered[j].size() != k || owner[j] != 1) {
      set_error("plan: landmark %d: %zu of %lld pairs, %zu of %lld rhs terms, %d owners", j, covered[j].size(), k * (k + 1) / 2, ccovered[j].size(), k, owner[j]);
      return OSH_ERR_DEVICE;
    }
  }
  for (int u : used) if (u != 1) { set_error("plan: a contribution slot is written %d times", u); return OSH_ERR_DEVICE; }
  for (int u : cused) if (u != 1) { set_error("plan: a rhs contribution slot is written %d times", u); return OSH_ERR_DEVICE; }
  stats[0] = (int64_t)plan.items.size(); stats[1] = plan.n_sym; stats[2] = (int64_t)plan.recs.size();
  stats[3] = (int64_t)plan.n_contrib; stats[4] = (int64_t)plan.n_ccontrib; stats[5] = plan.tile_steps; stats[6] = plan.pair_blocks;
  stats[7] = (int64_t)plan.rblk.size();
  return OSH_OK;
}

extern "C" int osh_lba_schur_plan_stats(const osh_lba_problem* p, int64_t stats[8]) { return osh_lba_schur_plan_stats_cut(p, 0, stats); }

// Landmarks per Schur item / edges per landmark chunk of a call of n_windows windows (the size classes of schur_plan.h:item_max_tier
// and lba_pack.h:chunk_edges_tier; use_env != 0: with the tuning aids OSH_LBA_ITEM_MAX / OSH_LBA_CHUNK_EDGES applied, as an upload does).
extern "C" int osh_lba_pack_cuts(int32_t n_windows, int use_env, int32_t cuts[2]) {
  if (n_windows <= 0 || !cuts) { set_error("osh_lba_pack_cuts: bad arguments"); return OSH_ERR_INVALID; }
  cuts[0] = use_env ? item_max_lm(n_windows) : item_max_tier(n_windows);
  cuts[1] = use_env ? chunk_max_edges(n_windows) : chunk_edges_tier(n_windows);
  return OSH_OK;
}
