// liba_pack_check.cpp -- host-only self check of the inertial BA packer (liba_pack.h).  Needs no GPU.
// Describes, bands, lays out and packs the problems exactly as liba_run (liba_device.hip) does, into a malloc'ed input arena instead
// of pinned staging, and verifies what k_liba relies on without looking: the window offsets, the landmark-major edge order with its
// left + right pairs, the pose-by-pose walk order, the (landmark, pose) -> block table, the link colours and the band.
#include "common.h"
#include "liba_pack.h"
#include <cstdlib>

using namespace osh;

extern "C" int osh_liba_pack_check(int32_t nw, const osh_liba_problem* pr, int64_t stats[8]) {
  if (nw <= 0 || !pr || !stats) { set_error("osh_liba_pack_check: bad arguments"); return OSH_ERR_INVALID; }
  const LibaKnobs knobs = liba_read_knobs();
  LibaPack pk;
  LibaPanels pan;
  LibaScratch sc;
  LibaLayout y;
  if (liba_describe(nw, pr, -1, -1.0, pk) != OSH_OK || liba_panels(pk, pan) != OSH_OK) { set_error("%s", pk.msg); return pk.err; }
  const bool banding = pan.NB != kLNB && !knobs.dense;
  if (banding) liba_band(nw, pr, pk, sc);
  liba_layout(nw, pk.tot, false, y);
  char* const base = static_cast<char*>(std::malloc(y.in.bytes));
  if (!base) { set_error("osh_liba_pack_check: out of memory"); return OSH_ERR_DEVICE; }
  auto done = [&](int code) { std::free(base); return code; };
  if (liba_pack(nw, pr, pk, y, base, sc) != OSH_OK) { set_error("%s", pk.msg); return done(pk.err); }
#define CHECK(cond, ...) do { if (!(cond)) { set_error(__VA_ARGS__); return done(OSH_ERR_DEVICE); } } while (0)
  // ---- every section inside its arena, one after another
  const size_t arena_bytes[3] = {y.in.bytes, y.out.bytes, y.work.bytes};
  size_t next[3] = {0, 0, 0};
  CHECK(y.n_ext == 52, "layout: %d sections recorded", y.n_ext);
  for (int k = 0; k < y.n_ext; ++k) {
    const LibaLayout::Extent& x = y.ext[k];
    CHECK(x.off % 256 == 0 && x.off >= next[x.arena] && x.off + std::max<size_t>(x.bytes, 8) <= arena_bytes[x.arena], "layout: section %d leaves its arena", k);
    next[x.arena] = x.off + std::max<size_t>(x.bytes, 8);
  }
  CHECK(std::memcmp(y.desc.in(base), pk.desc.data(), nw * sizeof(LibaDesc)) == 0, "the staged descriptors are not the packer's");
  LibaTotals run;
  long long merged = 0, colours_max = 0, n_il = 0;
  std::vector<char> used;
  std::vector<int> first, lo, hi;
  for (int w = 0; w < nw; ++w) {
    const osh_liba_problem& p = pr[w];
    const LibaDesc& d = pk.desc[w];
    const int N = d.N, L = d.L, E = d.E;
    // ---- sizes, and offsets = the running totals
    CHECK(N == p.n_opt && d.NV == N + p.n_fixed_imu && d.K == d.NV + p.n_fixed && L == p.n_points && E == p.n_edges && d.NL == p.n_links && d.n == 15 * N, "window %d: sizes", w);
    CHECK((size_t)d.pose_off == run.K && (size_t)d.vel_off == run.NV && (size_t)d.pt_off == run.L && (size_t)d.edge_off == run.E && (size_t)d.link_off == run.NL &&
          (size_t)d.lmoff_off == run.LO && (size_t)d.peloff_off == run.PO && (size_t)d.pel_off == run.EF && (size_t)d.lmpose_off == run.LP &&
          (size_t)d.H_off == run.Htot && (size_t)d.b_off == run.btot, "window %d: offsets are not the running totals", w);
    // ---- the state
    for (int k = 0; k < d.K; ++k) {
      const double* o = y.pose.in(base) + ((size_t)d.pose_off + k) * 24;
      CHECK(!std::memcmp(o, p.pose_Rcw + 9 * k, 72) && !std::memcmp(o + 9, p.pose_tcw + 3 * k, 24) && !std::memcmp(o + 12, p.pose_Rwb + 9 * k, 72) &&
            !std::memcmp(o + 21, p.pose_twb + 3 * k, 24), "window %d: pose of keyframe %d", w, k);
    }
    for (int k = 0; k < d.NV; ++k) {
      const double* o = y.vba.in(base) + ((size_t)d.vel_off + k) * 9;
      CHECK(!std::memcmp(o, p.vel + 3 * k, 24) && !std::memcmp(o + 3, p.bias_g + 3 * k, 24) && !std::memcmp(o + 6, p.bias_a + 3 * k, 24), "window %d: velocity / biases of keyframe %d", w, k);
    }
    CHECK(!L || !std::memcmp(y.pts.in(base) + (size_t)d.pt_off * 3, p.points, (size_t)L * 24), "window %d: landmarks", w);
    // ---- sorted edges: a permutation of the caller's, each with its caller edge's data; landmark-major, poses ascending, pairs
    const int *ep = y.e_pose.in(base) + d.edge_off, *el = y.e_point.in(base) + d.edge_off, *eo = y.e_orig.in(base) + d.edge_off;
    const unsigned char* ek = y.e_kind.in(base) + d.edge_off;
    const double *obs = y.e_obs.in(base) + (size_t)d.edge_off * 3, *info = y.e_info.in(base) + d.edge_off;
    const int* lmo = y.lm_off.in(base) + d.lmoff_off;
    used.assign(E, 0);
    size_t ef = 0;
    for (int x = 0; x < E; ++x) {
      const int e = eo[x];
      CHECK(e >= 0 && e < E && !used[e], "window %d: sorted edge %d has a bad caller index", w, x);
      used[e] = 1;
      CHECK(ep[x] == p.edge_pose[e] && el[x] == p.edge_point[e] && ek[x] == p.edge_kind[e] && info[x] == p.edge_info[e] &&
            !std::memcmp(obs + 3 * (size_t)x, p.edge_obs + 3 * (size_t)e, 24), "window %d: sorted edge %d is not its caller edge", w, x);
      if (ep[x] < N) ++ef;
    }
    CHECK(lmo[0] == 0 && lmo[L] == E, "window %d: landmark offsets do not tile the edges", w);
    first.assign((size_t)L * N, -1);   // first sorted edge of every (landmark, optimisable pose)
    for (int j = 0; j < L; ++j) {
      CHECK(lmo[j] <= lmo[j + 1], "window %d: landmark offsets descend at %d", w, j);
      for (int x = lmo[j]; x < lmo[j + 1]; ++x) {
        CHECK(el[x] == j, "window %d: sorted edge %d lies outside its landmark's range", w, x);
        if (x > lmo[j]) {
          CHECK(ep[x] >= ep[x - 1], "window %d: landmark %d: poses not ascending", w, j);
          if (ep[x] == ep[x - 1]) {
            CHECK(ek[x - 1] == OSH_EDGE_MONO && ek[x] == OSH_EDGE_RIGHT && !(x - 1 > lmo[j] && ep[x - 2] == ep[x]), "window %d: landmark %d: an equal pose that is no left + right pair", w, j);
            ++merged;
            continue;
          }
        }
        if (ep[x] < N) first[(size_t)j * N + ep[x]] = x;
      }
    }
    // ---- the pose-by-pose walk order
    const int *po = y.pel_off.in(base) + d.peloff_off, *pel = y.pel_edge.in(base) + d.edge_off;
    CHECK(po[0] == 0 && (size_t)po[N] == ef, "window %d: pel_off does not end at the optimisable-pose edges", w);
    used.assign(E, 0);
    for (int idx = 0; idx < E; ++idx) {
      CHECK(pel[idx] >= 0 && pel[idx] < E && !used[pel[idx]], "window %d: pel_edge is not a permutation (place %d)", w, idx);
      used[pel[idx]] = 1;
    }
    for (int i = 0; i < N; ++i) {
      CHECK(po[i] <= po[i + 1], "window %d: pel_off descends at pose %d", w, i);
      for (int idx = po[i]; idx < po[i + 1]; ++idx)
        CHECK(ep[pel[idx]] == i && (idx == po[i] || pel[idx] > pel[idx - 1]), "window %d: pose %d's edges are not its own in landmark order (place %d)", w, i, idx);
    }
    for (int idx = po[N]; idx < E; ++idx) CHECK(ep[pel[idx]] >= N, "window %d: an optimisable pose's edge among the fixed keyframes' (place %d)", w, idx);
    // ---- (landmark, pose) -> place of the pair's first edge, -1 where there is no edge
    const int* lmpe = y.lm_pose_edge.in(base) + d.lmpose_off;
    for (size_t k = 0; k < (size_t)L * N; ++k) {
      if (first[k] < 0) { CHECK(lmpe[k] == -1, "window %d: lm_pose_edge has an entry without an edge (landmark %zu, pose %zu)", w, k / N, k % N); continue; }
      const int i = (int)(k % N);
      CHECK(lmpe[k] >= po[i] && lmpe[k] < po[i + 1] && pel[lmpe[k]] == first[k], "window %d: lm_pose_edge of landmark %zu, pose %d is not the pair's first edge", w, k / N, i);
    }
    // ---- links and their colours
    const int *lp = y.link_prev.in(base) + d.link_off, *lc = y.link_cur.in(base) + d.link_off, *lb = y.link_bias.in(base) + d.link_off;
    const int* col = y.link_colour.in(base) + d.link_off;
    int n_col = 0;
    for (int l = 0; l < d.NL; ++l) {
      const size_t g = (size_t)d.link_off + l;
      CHECK(lp[l] == p.link_prev[l] && lc[l] == p.link_cur[l] && lb[l] == (p.link_bias ? p.link_bias[l] : p.link_prev[l]) && y.link_robust.in(base)[g] == p.link_robust[l],
            "window %d: link %d is not the caller's", w, l);
      CHECK(!std::memcmp(y.link_preint.in(base) + g * OSH_PREINT_FLOATS, p.link_preint + (size_t)l * OSH_PREINT_FLOATS, OSH_PREINT_FLOATS * 4) &&
            !std::memcmp(y.link_info.in(base) + g * 81, p.link_info + (size_t)l * 81, 648) && !std::memcmp(y.link_info_g.in(base) + g * 9, p.link_info_g + (size_t)l * 9, 72) &&
            !std::memcmp(y.link_info_a.in(base) + g * 9, p.link_info_a + (size_t)l * 9, 72), "window %d: record or information of link %d", w, l);
      CHECK(col[l] >= 0, "window %d: link %d has no colour", w, l);
      n_col = std::max(n_col, col[l] + 1);
      for (int l2 = 0; l2 < l; ++l2) {
        if (col[l2] != col[l]) continue;
        const int k1[3] = {lp[l], lc[l], lb[l]}, k2[3] = {lp[l2], lc[l2], lb[l2]};
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) CHECK(k1[a] != k2[b], "window %d: links %d and %d share keyframe %d and colour %d", w, l2, l, k1[a], col[l]);
      }
    }
    CHECK(d.n_colours == n_col, "window %d: n_colours %d, largest colour + 1 = %d", w, d.n_colours, n_col);
    colours_max = std::max<long long>(colours_max, n_col);
    // ---- the band
    if (d.il == 1) {
      CHECK(banding && N >= 32 && 15 * (d.bw_kf + 1) <= d.n / 2 && d.bw == 15 * (d.bw_kf + 1) - 1, "window %d: band %d (%d keyframes) of %d unknowns", w, d.bw, d.bw_kf, d.n);
      lo.assign(L, N); hi.assign(L, -1);
      for (int e = 0; e < E; ++e)
        if (p.edge_pose[e] < N) { int& a = lo[p.edge_point[e]]; int& b = hi[p.edge_point[e]]; a = std::min(a, p.edge_pose[e]); b = std::max(b, p.edge_pose[e]); }
      for (int j = 0; j < L; ++j) CHECK(hi[j] - lo[j] <= d.bw_kf, "window %d: landmark %d spans more keyframes than the band", w, j);
      for (int l = 0; l < d.NL; ++l) {
        int mn = lc[l], mx = lc[l];
        for (int a : {lp[l], lb[l]}) if (a < N) { mn = std::min(mn, a); mx = std::max(mx, a); }
        CHECK(mx - mn <= d.bw_kf, "window %d: link %d spans more keyframes than the band", w, l);
      }
      ++n_il;
    } else {
      CHECK(d.il == 0 && d.bw == d.n && d.bw_kf == N, "window %d: a dense window with a band", w);
    }
    run.K += d.K; run.NV += d.NV; run.L += L; run.E += E; run.NL += d.NL; run.Htot += (size_t)d.n * d.n; run.btot += d.n; run.LO += (size_t)L + 1;
    run.PO += (size_t)N + 1; run.EF += ef; run.LP += (size_t)L * N;
  }
  const LibaTotals& t = pk.tot;
  CHECK(run.K == t.K && run.NV == t.NV && run.L == t.L && run.E == t.E && run.NL == t.NL && run.Htot == t.Htot && run.btot == t.btot && run.LO == t.LO &&
        run.PO == t.PO && run.EF == t.EF && run.LP == t.LP, "the totals are not the sums over the windows");
#undef CHECK
  stats[0] = (int64_t)t.E; stats[1] = (int64_t)t.EF; stats[2] = merged; stats[3] = colours_max; stats[4] = n_il;
  stats[5] = (int64_t)(y.in.bytes + y.out.bytes + y.work.bytes); stats[6] = pan.NB; stats[7] = pan.W;
  return done(OSH_OK);
}
