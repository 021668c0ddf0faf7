"""CPU checks of the 4-DoF pose graph (OptimizeEssentialGraph4DoF): the algebra header csrc/pgo4_se3.h compiled for the host
against pgo4_numpy.py, the C-ABI mirror, the synthetic walk's edge rules and the refusals that need no device."""
import ctypes as C

import numpy as np
import pytest

import pgo4_numpy as p4
from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_pgo as sp
from orb_slam3_study_kr_amd.pgo import INFO_4DOF


def _apply(op, n, a, b=None, c=None, width=None):
    lib = capi.load_host_library()
    a = np.ascontiguousarray(a, dtype=np.float64)
    arr = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (b, c)]
    out = np.zeros((n, width))
    p = lambda x: None if x is None else capi.ptr(x, capi.c_double_p)
    assert lib.osh_host_pgo4_apply(op, n, p(a), p(arr[0]), p(arr[1]), p(out)) == 0
    return out


def _rand_rot(rng, n, scale=1.0):
    w = rng.normal(0, scale, (n, 3))
    return p4.exp_so3(w)


def _states(rng, n, its=None):
    Rwb0 = _rand_rot(rng, n)
    st = dict(DR=p4.exp_so3(np.c_[np.zeros(n), np.zeros(n), rng.normal(0, 0.3, n)]), Rwb=None, twb=rng.normal(0, 3, (n, 3)),
              Rcw=_rand_rot(rng, n), tcw=rng.normal(0, 3, (n, 3)),
              its=np.asarray(its if its is not None else rng.integers(0, 5, n), np.int64))
    st["Rwb"] = p4.m3_mul(st["DR"], Rwb0)
    Rcb = _rand_rot(rng, n, 0.2)
    tcb = rng.normal(0, 0.1, (n, 3))
    return st, Rwb0, Rcb, tcb


def _consts(Rwb0, Rcb, tcb):
    n = len(tcb)
    return np.concatenate([Rwb0.reshape(n, 9), Rcb.reshape(n, 9), tcb], 1)


def test_struct_sizes_match_header():
    lib = capi.load_host_library()
    out = np.zeros(2, np.int64)
    lib.osh_host_pgo4_sizes(capi.ptr(out, capi.c_int64_p))
    assert out[0] == C.sizeof(capi.Pgo4Problem)
    assert out[1] == C.sizeof(capi.Pgo4Result)
    assert "osh_pgo4_solve" in capi.EXPORTED_SYMBOLS and "osh_pgo4_linearize" in capi.EXPORTED_SYMBOLS


def test_small_angle_exp_and_normalize_are_bitwise():
    """libm-free paths (the d < 1e-5 branch of ExpSO3, the Newton polar factor) agree with numpy to the bit."""
    rng = np.random.default_rng(1)
    w = rng.normal(0, 3e-6, (200, 3))
    w[:50, :2] = 0                                    # the yaw-only updates of the 4-DoF vertex
    assert np.array_equal(_apply(capi.OSH_PGO4_EXP, len(w), w, width=9), p4.exp_so3(w).reshape(-1, 9))
    R = (_rand_rot(rng, 100) + rng.normal(0, 1e-3, (100, 3, 3))).reshape(-1, 9)
    assert np.array_equal(_apply(capi.OSH_PGO4_NORMALIZE, 100, R, width=9), p4.normalize_rotation(R).reshape(-1, 9))


def test_large_angle_exp_matches_long_double():
    p4.require_extended()
    rng = np.random.default_rng(2)
    w = rng.normal(0, 1.0, (200, 3))
    got = _apply(capi.OSH_PGO4_EXP, len(w), w, width=9).reshape(-1, 3, 3)
    ref = p4.exp_so3(w, np.longdouble).astype(np.float64)
    assert np.abs(got - ref).max() <= 4e-16
    assert np.abs(got - p4.exp_so3(w)).max() <= 4e-16


def test_update_w_through_the_normalisation():
    """UpdateW bit for bit with small yaw steps (libm-free), at every update count: its == 4 runs the DR normalisation."""
    rng = np.random.default_rng(3)
    n = 250
    st, Rwb0, Rcb, tcb = _states(rng, n, its=np.arange(n) % 5)
    u = np.c_[rng.normal(0, 3e-6, n), rng.normal(0, 1e-2, (n, 3))]
    got = p4.unpack_state(_apply(capi.OSH_PGO4_UPDATE, n, p4.pack_state(st), _consts(Rwb0, Rcb, tcb), u, width=34))
    ref = p4.update_w(st, Rwb0, Rcb, tcb, u)
    for k in ("DR", "Rwb", "twb", "Rcw", "tcw", "its"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got["its"], np.where(st["its"] == 4, 0, st["its"] + 1))
    normed = st["its"] == 4
    assert np.all(got["DR"][normed][:, 2, :2] == 0) and np.all(got["DR"][normed][:, :2, 2] == 0)


def test_update_w_large_yaw_matches_long_double():
    p4.require_extended()
    rng = np.random.default_rng(4)
    n = 250
    st, Rwb0, Rcb, tcb = _states(rng, n, its=np.arange(n) % 5)
    u = np.c_[rng.normal(0, 0.5, n), rng.normal(0, 1e-1, (n, 3))]
    got = p4.unpack_state(_apply(capi.OSH_PGO4_UPDATE, n, p4.pack_state(st), _consts(Rwb0, Rcb, tcb), u, width=34))
    ref = p4.update_w({k: (v.astype(np.longdouble) if k != "its" else v) for k, v in st.items()}, Rwb0, Rcb, tcb, u, np.longdouble)
    for k in ("DR", "Rwb", "Rcw"):
        assert np.abs(got[k] - ref[k].astype(np.float64)).max() <= 2e-15, k
    for k in ("twb", "tcw"):
        assert np.abs(got[k] - ref[k].astype(np.float64)).max() <= 2e-14, k
    assert np.array_equal(got["its"], ref["its"])


@pytest.mark.parametrize("branch", ["outside", "small_sin", "general"])
def test_edge_error_over_the_log_branches(branch):
    rng = np.random.default_rng(5)
    n = 100
    si, _, _, _ = _states(rng, n)
    sj = dict(si)
    sj["Rcw"], sj["tcw"] = _rand_rot(rng, n), rng.normal(0, 3, (n, 3))
    A = p4.m3_mul_bt(si["Rcw"], sj["Rcw"])
    if branch == "outside":        # cos theta > 1 on every row: Rcw_j = Rcw_i and dR = I (1 + 1e-12)
        sj["Rcw"] = si["Rcw"].copy()
        dR = np.broadcast_to(np.eye(3) * (1 + 1e-12), (n, 3, 3)).copy()
    elif branch == "small_sin":    # residual rotation below 1e-5
        dR = p4.m3_mul(p4.exp_so3(rng.normal(0, 1e-7, (n, 3))), A)
    else:
        dR = p4.m3_mul(p4.exp_so3(rng.normal(0, 0.5, (n, 3))), A)
    dt = rng.normal(0, 1, (n, 3))
    meas = np.concatenate([dR.reshape(n, 9), dt], 1)
    got = _apply(capi.OSH_PGO4_EDGE_ERROR, n, meas, p4.pack_state(si), p4.pack_state(sj), width=6)
    ref = p4.edge_error(dR, dt, si["Rcw"], si["tcw"], sj["Rcw"], sj["tcw"])
    B = p4.m3_mul_bt(p4.m3_mul_bt(si["Rcw"], sj["Rcw"]), dR)
    c = (B[:, 0, 0] + B[:, 1, 1] + B[:, 2, 2] - 1.0) * 0.5
    if branch == "outside":
        assert np.all(np.abs(c) > 1)
    if branch == "small_sin":
        assert np.all(np.abs(np.sin(np.arccos(np.clip(c, -1, 1)))) < 1e-5)
    if branch == "general":
        assert np.abs(got - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
        p4.require_extended()
        ld = p4.edge_error(dR, dt, si["Rcw"], si["tcw"], sj["Rcw"], sj["tcw"], np.longdouble).astype(np.float64)
        assert np.abs(got - ld).max() <= 1e-13
    else:
        assert np.array_equal(got, ref)   # no libm on these branches


def test_unknown_op_and_missing_arrays_are_refused():
    lib = capi.load_host_library()
    a, out = np.zeros(34), np.zeros(34)
    p = lambda x: capi.ptr(x, capi.c_double_p)
    assert lib.osh_host_pgo4_apply(9, 1, p(a), None, None, p(out)) == -1
    assert lib.osh_host_pgo4_apply(capi.OSH_PGO4_UPDATE, 1, p(a), None, None, p(out)) == -1


# ---- the synthetic walk (pack_loop4): the edge rules of src/Optimizer.cc:5300-5470 ----
def _pairs(m, g, kfs):
    return [(kfs[a], kfs[b]) for a, b in g.edge_ij]


def test_pack_loop4_edge_rules():
    m = sp.make_inertial_loop(40, seed=3, earlier_loop=True)
    g, kfs, vScw = sp.pack_loop4(m)
    pairs = _pairs(m, g, kfs)
    # the loop connections come first, in map then set order; the (cur, loop) pair is kept below minFeat
    assert m.weight(m.cur, m.loop) < sp.MIN_FEAT
    assert (m.cur, m.loop) in pairs[:sum(len(s) for s in m.connections.values())]
    # every chain keyframe has its inertial edge to mPrevKF, and there is no parent edge beyond those
    for i in range(1, m.n):
        assert (i, i - 1) in pairs
    assert len(set(pairs)) < len(pairs)     # a loop connection that is also the mPrevKF pair stays doubled
    # covisibility edges never join mPrevKF / mNextKF / children / loop edges, and never repeat a loop connection
    conn = {(min(m.kf_id[i], m.kf_id[j]), max(m.kf_id[i], m.kf_id[j])) for i in m.connections for j in m.connections[i]}
    n_conn = sum(1 for i in m.connections for j in m.connections[i] if m.weight(i, j) >= sp.MIN_FEAT or (i, j) == (m.cur, m.loop))
    for i, j in pairs[n_conn:]:
        if j == i - 1 and m.prev_kf[i] == j:
            continue
        if j in m.loop_set(i):
            continue
        assert (min(m.kf_id[i], m.kf_id[j]), max(m.kf_id[i], m.kf_id[j])) not in conn
        assert m.parent[j] != i and m.kf_id[j] < m.kf_id[i] and m.weight(i, j) >= sp.MIN_FEAT
    # the earlier loop edge (n/2, 2) is inserted once, as a loop edge, although it is also covisible
    assert pairs.count((m.n // 2, 2)) == 1
    # only pLoopKF is fixed; the information is the reference's diagonal
    assert [kfs[k] for k in np.flatnonzero(g.fixed)] == [m.loop]
    assert tuple(g.info_diag) == INFO_4DOF == (1e3, 1e3, 1.0, 1.0, 1.0, 1.0)


def test_pack_loop4_vertex_states():
    m = sp.make_inertial_loop(30, seed=4)
    g, kfs, vScw = sp.pack_loop4(m)
    for v, i in enumerate(kfs):
        if i in m.corrected:       # ImuCamPose(Rwc, twc, pKF) from CorrectedSim3^-1
            Rcw = sp._quat_to_R(m.corrected[i][:4])
            assert np.allclose(g.Rcw[v], Rcw, atol=1e-12)
            assert np.allclose(g.Rwb[v], Rcw.T @ g.Rcb[v], atol=1e-12)
        else:                      # ImuCamPose(pKF): the float pose and the float IMU pose
            assert np.array_equal(g.Rcw[v], g.Rcw[v].astype(np.float32).astype(np.float64))
            assert np.array_equal(g.twb[v], g.twb[v].astype(np.float32).astype(np.float64))
    assert not np.allclose(g.Rcb[0], np.eye(3))


def test_pack_loop4_skips_a_bad_keyframe():
    m = sp.make_inertial_loop(30, seed=5)
    m.bad[10] = True
    g, kfs, _ = sp.pack_loop4(m)
    assert 10 not in kfs and len(kfs) == m.n - 1
    assert all(10 not in (kfs[a], kfs[b]) for a, b in g.edge_ij)


# ---- the host layer's walk (csrc/host/OptimizerEssentialGraph4DoF.cc) against pack_loop4 ----
def _edge_set(g, ids):
    """Edges as (mnId i, mnId j, dR, dt), sorted: LoopConnections and GetAllKeyFrames iterate in pointer order in the host."""
    rows = [(int(ids[a]), int(ids[b]), tuple(np.round(np.r_[R.ravel(), t], 9))) for (a, b), R, t in zip(g.edge_ij, g.dR, g.dt)]
    return sorted(rows)


def _odd_map(n=40, seed=3, n_points=0):
    """An inertial loop where mNextKF and a child have lower ids than a keyframe they are covisible with, so that only the
    mNextKF / hasChild exclusions keep those covisibility edges out."""
    m = sp.make_inertial_loop(n, seed=seed, earlier_loop=True, n_points=n_points)
    m.prev_kf[8] = 20          # keyframe 20's mNextKF is keyframe 8
    m.prev_kf[21] = 19
    m.parent[5] = 20           # keyframe 5 is a child of keyframe 20

    def connect(a, b, w):
        m.cov[a] = [(o, x) for o, x in m.cov[a] if o != b] + [(b, w)]
        m.cov[b] = [(o, x) for o, x in m.cov[b] if o != a] + [(a, w)]

    connect(20, 8, 150)
    connect(20, 5, 150)
    return m


@pytest.mark.parametrize("odd", [False, True])
def test_host_pack4_matches_pack_loop4(odd):
    m = _odd_map() if odd else sp.make_inertial_loop(60, seed=5, earlier_loop=True)
    with sp.HostPgo4Map(m) as h:
        hg, ids = h.pack4()
        g, kfs, _ = sp.pack_loop4(m, kf_pose=h.kf_poses())   # the poses as the stand-in keeps them (unit quaternions)
    assert np.array_equal(ids, m.kf_id[kfs])
    assert np.array_equal(hg.fixed, g.fixed) and [kfs[v] for v in np.flatnonzero(hg.fixed)] == [m.loop]
    # vertex states: the corrected ones from CorrectedSim3, the others the float pose / IMU pose (the stand-in's float Tcb
    # round trip differs from the generator's by float rounding)
    for k, tol in (("Rwb", 2e-6), ("twb", 2e-5), ("Rcw", 2.5e-7), ("tcw", 1e-12), ("Rcb", 2e-7), ("tcb", 2e-8)):
        assert np.abs(getattr(hg, k) - getattr(g, k)).max() <= tol, k
    he, pe = _edge_set(hg, ids), _edge_set(g, m.kf_id[kfs])
    assert [e[:2] for e in he] == [e[:2] for e in pe]
    assert np.abs(np.array([e[2] for e in he]) - np.array([e[2] for e in pe])).max() <= 2e-9
    pairs = [(int(ids[a]), int(ids[b])) for a, b in hg.edge_ij]
    kid = lambda i: int(m.kf_id[i])  # noqa: E731
    assert (kid(m.cur), kid(m.loop)) in pairs and m.weight(m.cur, m.loop) < sp.MIN_FEAT
    assert len(set(pairs)) < len(pairs)                         # doubled pairs stay separate edges
    assert pairs.count((kid(m.n // 2), kid(2))) == 1            # loop edge, not repeated as covisibility
    inserted = {(min(kid(i), kid(j)), max(kid(i), kid(j))) for i in m.connections for j in m.connections[i]
                if m.weight(i, j) >= sp.MIN_FEAT or (i, j) == (m.cur, m.loop)}
    n_conn = sum(1 for i in m.connections for j in m.connections[i] if m.weight(i, j) >= sp.MIN_FEAT or (i, j) == (m.cur, m.loop))
    prev_pairs = {(kid(i), kid(int(m.prev_kf[i]))) for i in range(m.n) if m.prev_kf[i] >= 0}
    normal = sorted(pairs)
    for p in inserted:         # sInsertedEdges: a covisible pair already joined by a loop connection is not added again
        extra = normal.count(p) + normal.count(p[::-1]) - sum(1 for q in prev_pairs if q in (p, p[::-1]))
        assert extra <= sum(1 for i in m.connections for j in m.connections[i] if {kid(i), kid(j)} == set(p)), p
    assert len(pairs) >= n_conn
    if odd:
        assert (kid(20), kid(8)) not in pairs and (kid(8), kid(20)) in pairs    # mNextKF: only the inertial edge of keyframe 8
        assert (kid(20), kid(5)) not in pairs                                   # child
    assert not any(ids[b] > ids[a] for (a, b), p in zip(hg.edge_ij, pairs) if p not in prev_pairs and
                   (min(p), max(p)) not in inserted)                            # covisibility / loop edges point to lower ids


def test_host_pack4_skips_a_bad_keyframe():
    m = sp.make_inertial_loop(30, seed=5)
    m.bad[10] = True
    g, kfs, _ = sp.pack_loop4(m)
    with sp.HostPgo4Map(m) as h:
        hg, ids = h.pack4()
    assert m.kf_id[10] not in ids and len(ids) == m.n - 1
    assert _edge_set(hg, ids)[0][:2] == _edge_set(g, m.kf_id[kfs])[0][:2] and len(hg.edge_ij) == len(g.edge_ij)


def test_host_run4_over_the_limit_leaves_the_map_untouched(capfd):
    m = sp.make_inertial_loop(capi.OSH_PGO_MAX_VERTICES + 2, seed=2, n_points=20)   # 4001 free keyframes
    with sp.HostPgo4Map(m) as h:
        poses, pts = h.kf_poses(), h.mp_positions()
        assert h.run4() == 0
        assert np.array_equal(h.kf_poses(), poses) and np.array_equal(h.mp_positions(), pts)
        assert h.change_index() == 0 and not h.normal_updates().any()
    assert "OptimizeEssentialGraph4DoF: 4001 keyframes to optimise" in capfd.readouterr().err
