"""Schur items of up to 256 landmarks, what a call of more than 128 windows cuts (csrc/schur_plan.h:item_max_lm): one wavefront of
k_schur_fused walks up to 32 chunks of an item, and the device packer (csrc/lba_pack_device.hip) numbers up to 256 records per item.
Four small windows, each cut at 256 on its own through OSH_LBA_ITEM_MAX (read once per upload): 3, 5 and 8 optimisable keyframes whose
largest observer sets hold more than 256 landmarks -- items of 9, 17 and 32 chunks, a long item in each of the 16 x 4, 12 x 5 and 8 x 8
lane mappings, partial last chunks -- and 12 keyframes with tracks of 9-12 observers, whose cross items ride along (asserted on the
CPU plan, so that a change of synth cannot hollow the test out).
  * both packers give the same bytes at caps 65, 128 and 256 (the comparison of tests/test_gpu_pack.py);
  * S and b_s of one trial at 256 against the CPU oracle at the bounds tests/test_gpu_schur_blocks.py uses at 64, the same windows at
    64 as the control, the two against each other at those bounds, and the whole optimize(): the same iterations and trials, poses and
    landmarks within the end-to-end bounds of tests/test_gpu_pack.py;
  * a window solved in a call cut at 256 has the same bits wherever it stands in the call, whatever the other windows are, and from
    run to run (the property of tests/test_gpu_schur_reduce.py), in a 12-window call."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import lba, synth

pytestmark = pytest.mark.gpu

LAMBDA = 1e-3
LANES = {nx: 16 if nx <= 4 else (12 if nx == 5 else 8) for nx in range(1, 9)}   # landmarks per chunk of a symmetric item of nx row poses
SPECS = {
    3: dict(seed=9301, n_free=3, n_fixed=1, n_points=500, track_len=(3, 4)),
    5: dict(seed=9302, n_free=5, n_fixed=1, n_points=620, track_len=(5, 6)),
    8: dict(seed=9303, n_free=8, n_fixed=1, n_points=600, track_len=(8, 9)),
    12: dict(seed=9304, n_free=12, n_fixed=1, n_points=500, track_len=(9, 12)),
}
NS = sorted(SPECS)


def _window(n):
    sp = dict(SPECS[n])
    return synth.make_window(sp.pop("seed"), stereo=True, **sp)


def _run(solver, ws):
    """S, b_s of one trial and the result of optimize() of every window of the batch ``ws``."""
    solver.upload(ws)
    trials = [solver.debug_trial(k, LAMBDA)[:2] for k in range(len(ws))]
    solver.optimize()
    return [(S, bs, r) for (S, bs), r in zip(trials, solver.download())]


def _assert_same_bits(a, b):
    (Sa, bsa, ra), (Sb, bsb, rb) = a, b
    iu = np.triu_indices(Sa.shape[0])
    np.testing.assert_array_equal(Sa[iu], Sb[iu])
    np.testing.assert_array_equal(bsa, bsb)
    assert (ra.iterations, ra.trials) == (rb.iterations, rb.trials) and ra.iterations > 0
    np.testing.assert_array_equal(ra.trials_trace, rb.trials_trace)
    np.testing.assert_array_equal(ra.chi2_trace, rb.chi2_trace)
    np.testing.assert_array_equal(ra.lambda_trace, rb.lambda_trace)
    np.testing.assert_array_equal(ra.pose_qt, rb.pose_qt)
    np.testing.assert_array_equal(ra.points, rb.points)


@pytest.fixture(scope="module")
def windows():
    return {n: _window(n) for n in NS}


def _alone(windows, cap):
    """n -> (S, b_s, result, plan statistics) of the window uploaded alone, cut at ``cap`` landmarks per item and, like a large batch, at
    1024 edges per landmark chunk"""
    mp = pytest.MonkeyPatch()
    mp.setenv("OSH_LBA_ITEM_MAX", str(cap))
    mp.setenv("OSH_LBA_CHUNK_EDGES", "1024")
    try:
        out = {}
        with lba.LbaSolver(0) as s:
            for n in NS:
                S, bs, r = _run(s, [windows[n]])[0]
                out[n] = (S, bs, r, s.plan_stats())
        return out
    finally:
        mp.undo()


@pytest.fixture(scope="module")
def at256(hip_lib, windows):
    return _alone(windows, 256)


@pytest.fixture(scope="module")
def at64(hip_lib, windows):
    return _alone(windows, 64)


def test_the_windows_hold_the_long_items(windows):
    sym, cross = {}, {}
    for n in NS:
        for (s, nx, ny, lm), c in lba.schur_plan_shapes(windows[n], 256)[0].items():
            (sym if s else cross).setdefault((nx, ny), []).append(lm)
    chunks = lambda nx, lm: -(-lm // LANES[nx])
    long_items = {(LANES[nx], chunks(nx, lm), lm) for (nx, _), lms in sym.items() for lm in lms if lm > 64}
    assert {c for _, c, _ in long_items} >= {9, 17, 32}, sorted(long_items)
    for nx, lanes, most in ((3, 16, 16), (5, 12, 22), (8, 8, 32)):       # the longest item of each mapping: 256 landmarks
        mine = [lm for lm in sym[(nx, nx)] if lm > 64]
        assert 256 in mine and chunks(nx, 256) == most
        assert any(lm % lanes for lm in mine), (nx, mine)                  # a partial last chunk in a long item
    assert any(lm > 64 for lms in cross.values() for lm in lms) and all(nx == 8 for nx, _ in cross)
    k12 = np.bincount(windows[12].edge_point[windows[12].edge_pose < 12], minlength=windows[12].n_points)
    assert 9 <= k12.max() <= 12 and all(not any(s == 0 for (s, *_) in lba.schur_plan_shapes(windows[n], 256)[0]) for n in (3, 5, 8))


@pytest.mark.parametrize("cap", [65, 128, 256])
def test_both_packers_give_the_same_bytes(hip_lib, windows, cap, monkeypatch):
    monkeypatch.setenv("OSH_LBA_ITEM_MAX", str(cap))
    ws = [windows[n] for n in NS] + [synth.make_window(9310, n_free=4, n_fixed=2, n_points=450, stereo=False, track_len=(2, 6), obs_dropout=0.1),
                                     synth.make_window(9311, n_free=2, n_fixed=1, n_points=300, stereo=True, track_len=(2, 3))]
    with lba.LbaSolver(0) as s:
        st = s.pack_compare(ws)
        n_items = sum(sum(lba.schur_plan_shapes(w, cap)[0].values()) for w in ws)
        assert st["items"] == n_items and st["records"] >= sum(w.n_points for w in ws)
        # and the same optimisation from either packing
        out = []
        for mode in (0, 1):
            s.set_pack_mode(mode)
            out.append(s.solve(ws))
        for a, b in zip(*out):
            assert (a.iterations, a.trials) == (b.iterations, b.trials)
            assert np.array_equal(a.pose_qt, b.pose_qt) and np.array_equal(a.points, b.points) and np.array_equal(a.edge_chi2, b.edge_chi2)


@pytest.mark.parametrize("n", NS)
def test_the_cut_was_applied(windows, at256, at64, n):
    for got, cap in ((at256, 256), (at64, 64)):
        want = lba.schur_plan_check(windows[n], cap)
        st = got[n][3]
        assert (st["items"], st["sym_items"], st["contributions"], st["rhs_contributions"]) == \
               (want["items"], want["sym_items"], want["contributions"], want["rhs_contributions"])
    assert at256[n][3]["items"] < at64[n][3]["items"] and at256[n][3]["contributions"] < at64[n][3]["contributions"]


@pytest.mark.parametrize("cap", [256, 64])
@pytest.mark.parametrize("n", NS)
def test_one_trial_against_the_oracle(windows, at256, at64, n, cap):
    from oracle import binding as ob
    S, bs = (at256 if cap == 256 else at64)[n][:2]
    So, bso, _ = ob.lba_schur_step(windows[n], LAMBDA)
    iu = np.triu_indices(S.shape[0])
    np.testing.assert_allclose(S[iu], So[iu], rtol=1e-10, atol=1e-11 * np.abs(So).max())
    np.testing.assert_allclose(bs, bso, rtol=1e-10, atol=1e-11 * np.abs(bso).max())


@pytest.mark.parametrize("n", NS)
def test_items_of_256_against_items_of_64(at256, at64, n):
    (S, bs, r, _), (S0, bs0, r0, _) = at256[n], at64[n]
    iu = np.triu_indices(S.shape[0])
    np.testing.assert_allclose(S[iu], S0[iu], rtol=1e-10, atol=1e-11 * np.abs(S0[iu]).max())   # (the device fills the upper triangle only)
    np.testing.assert_allclose(bs, bs0, rtol=1e-10, atol=1e-11 * np.abs(bs0).max())
    assert (r.iterations, r.trials) == (r0.iterations, r0.trials) and r.iterations > 0
    np.testing.assert_array_equal(r.trials_trace, r0.trials_trace)
    # the end-to-end bounds between two size classes of tests/test_gpu_pack.py
    np.testing.assert_allclose(r.pose_qt, r0.pose_qt, rtol=0, atol=1e-9)
    np.testing.assert_allclose(r.points, r0.points, rtol=0, atol=1e-8)
    np.testing.assert_allclose(r.edge_chi2, r0.edge_chi2, rtol=1e-6, atol=1e-9)


def test_the_same_bits_wherever_the_window_stands_in_the_call(hip_lib, windows):
    fill = [synth.make_window(9320 + k, n_free=2 + k, n_fixed=1 + k % 2, n_points=120 + 40 * k, stereo=bool(k % 2), track_len=(2, 4 + k)) for k in range(8)]
    other = [synth.make_window(9340 + k, n_free=9 - k, n_fixed=2, n_points=400 - 30 * k, stereo=True, track_len=(3, 9)) for k in range(8)]
    mine = [windows[n] for n in NS]
    mp = pytest.MonkeyPatch()
    mp.setenv("OSH_LBA_ITEM_MAX", "256")      # a 12-window call cuts its chunks at 1024 edges as every larger call does
    try:
        with lba.LbaSolver(0) as s:
            base = _run(s, mine + fill)
            again = _run(s, mine + fill)
            rev = _run(s, (mine + fill)[::-1])
            rot = _run(s, [(mine + fill)[(k + 5) % 12] for k in range(12)])
            among_others = _run(s, other[:3] + mine[:2] + other[3:6] + mine[2:] + other[6:])
    finally:
        mp.undo()
    for k in range(12):
        _assert_same_bits(again[k], base[k])
        _assert_same_bits(rev[11 - k], base[k])
        _assert_same_bits(rot[(k - 5) % 12], base[k])
    for k, pos in enumerate((3, 4, 8, 9)):
        _assert_same_bits(among_others[pos], base[k])
