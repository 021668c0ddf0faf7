"""Stage checks of the pose-inertial kernel (k_posei, csrc/posei_device.hip) that the end-to-end parity of test_gpu_posei.py cannot
make: the system of the first Gauss-Newton iteration on its own (osh_posei_linearize against the oracle's posei_linearize), and the
kernel's global-memory edge path (a batch whose largest frame has more than 1400 edges keeps no frame's edges in LDS).

The bound of the system comparison is computed at run time: 2 x the change of the ORACLE's own output when the float32
preintegration record moves by one float32 ulp per entry (liba_stage_numpy.noise_floor; 2 because device and host libm may differ at
more than one sinf / cosf), never more than the caps 1e-6 (H scaled by its diagonal) and 5e-6 (b relative to its largest entry).

Measured on an MI355X, device distance | bound (2 x noise floor); the tests print these lines (-s):
    frame        edges   scaled H                  b
    stereo-m0       60   4.42e-11 | 1.96e-10   1.09e-08 | 2.77e-06
    mono-m0         60   6.49e-11 | 2.31e-10   1.42e-08 | 2.48e-06
    fisheye-m0      60   6.49e-11 | 2.31e-10   1.42e-08 | 2.48e-06
    rig-m0          60   4.42e-11 | 1.96e-10   1.09e-08 | 2.77e-06
    stereo-m1       60   3.39e-10 | 4.45e-07   1.01e-10 | 5.94e-07
    mono-m1         60   1.17e-12 | 4.46e-07   3.03e-10 | 6.07e-07
    fisheye-m1      60   1.17e-12 | 4.46e-07   3.03e-10 | 6.07e-07
    rig-m1          60   3.39e-10 | 4.45e-07   1.01e-10 | 5.94e-07
    n1344-m0      1344   4.45e-11 | 4.39e-10   1.93e-08 | 4.47e-06      (cached, the frame fills its ecap)
    n1344-m1      1344   1.32e-12 | 4.47e-07   5.99e-11 | 1.41e-07
    n1400-m0      1400   3.91e-16 | 4.34e-10   1.17e-16 | 3.76e-06      (cached, ecap 1408)
    n1400-m1      1400   3.70e-16 | 4.48e-07   1.80e-16 | 1.42e-07
    n1401-m0      1401   1.75e-11 | 2.27e-10   9.12e-09 | 4.17e-06      (global memory)
    n1401-m1      1401   4.72e-16 | 4.48e-07   3.58e-16 | 1.42e-07
The 60-edge frame has the same bits alone (LDS) and in a batch with a 1401-edge frame (global memory), at either place in the batch.
"""
import numpy as np
import pytest

import liba_stage_cases as lc
import liba_stage_numpy as ls
from orb_slam3_study_kr_amd import lba
from orb_slam3_study_kr_amd import synth_inertial as si
from test_gpu_posei import _check

pytestmark = pytest.mark.gpu

K_POSEI_MAX_CACHED = 1400      # csrc/posei_device.hip: the largest frame whose edges the block keeps in LDS


@pytest.fixture(scope="module")
def solver(hip_lib):
    with lba.LbaSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


def _assert_system(solver, ob, name):
    f = lc.frame(name)
    H, b = solver.linearize_pose_inertial(f)
    Hr, br = ob.posei_linearize(f)
    nf = ls.noise_floor(lc.posei_system(ob), f, "preint", lc.POSEI_MEASURES)
    bound_h, bound_b = min(2 * nf["H"], lc.CAP_H), min(2 * nf["b"], lc.CAP_B)
    dh, db = ls.scaled_h(H, Hr), ls.rel_max(b, br)
    print(f"\n    {name:12s} E {f.n_edges:5d}  scaled H {dh:.2e} | {bound_h:.2e}   b {db:.2e} | {bound_b:.2e}")
    assert 2 * nf["H"] <= lc.CAP_H and 2 * nf["b"] <= lc.CAP_B          # the bound cannot hide a 1e-4 error of a block
    assert dh <= bound_h and db <= bound_b, (name, dh, bound_h, db, bound_b)


@pytest.mark.parametrize("name", [n for n in lc.FRAMES if not n.startswith("n")])
def test_first_system_matches_the_oracle(solver, ob, name):
    _assert_system(solver, ob, name)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n", [1344, 1400, 1401])
def test_cached_and_global_memory_edge_paths(solver, ob, n, mode):
    """1400 edges: the largest cached frame (ecap 1408); 1401: every accessor goes to global memory; 1344 = 21 x 64: the frame fills
    its ecap exactly.  The first system, then the whole optimisation with the checks of test_gpu_posei.py."""
    f = lc.frame(f"n{n}-m{mode}")
    ecap = ((n + 63) & ~63) if n <= K_POSEI_MAX_CACHED else 0            # as osh_posei_optimize sizes the LDS planes
    assert f.n_edges == n and ecap == {1344: 1344, 1400: 1408, 1401: 0}[n]
    _assert_system(solver, ob, f"n{n}-m{mode}")
    ref = ob.posei_optimize(f)
    assert ref.rounds == 4 and ref.n_inliers > 1100
    _check(solver.optimize_poses_inertial([f])[0], ref, f)


@pytest.mark.parametrize("mode", [0, 1])
def test_a_frame_gives_the_same_bits_cached_and_from_global_memory(solver, mode):
    """The 60-edge frame alone (its edges in LDS) and beside a 1401-edge frame (no frame of that batch is cached).  The accessors return
    the same values in the same order and every sum has a fixed order, so every output has the same bits."""
    small, big = lc.frame(f"stereo-m{mode}"), lc.frame(f"n1401-m{mode}")
    alone = solver.optimize_poses_inertial([small])[0]
    for batch, k in (([small, big], 0), ([big, small], 1)):               # edge offset 0 and 1401 in the batch's arrays
        got = solver.optimize_poses_inertial(batch)[k]
        for fld in ("Rcw", "tcw", "Rwb", "twb", "vel", "bias_g", "bias_a", "H", "edge_chi2", "outlier"):
            np.testing.assert_array_equal(getattr(got, fld), getattr(alone, fld), err_msg=fld)
        assert (got.n_bad, got.n_inliers, got.rounds) == (alone.n_bad, alone.n_inliers, alone.rounds)


def test_recovery_pass_and_rec_init_through_the_global_arrays(solver, ob):
    """The 25-point frames of test_gpu_posei.py's recovery case in a batch with an uncached frame: setLevel / setOutlier / setChi of
    the classification and of the recovery pass write global memory."""
    frames = [si.make_posei_frame(24, mode=0, n_points=25, outlier_frac=0.3),                    # < 30 inliers: recovery pass
              lc.frame("n1401-m1"),
              si.make_posei_frame(25, mode=0, n_points=25, outlier_frac=0.3, rec_init=True),
              si.make_posei_frame(26, mode=0, n_points=5, outlier_frac=0.0)]                     # < 10 graph edges: one round
    refs = [ob.posei_optimize(f) for f in frames]
    assert refs[0].n_inliers < 30 and refs[2].n_inliers < 30
    got = solver.optimize_poses_inertial(frames)
    for g, r, f in zip(got, refs, frames):
        _check(g, r, f)
    assert got[3].rounds == 1
    cached = solver.optimize_poses_inertial([frames[0], frames[2], frames[3]])
    for g, c in zip((got[0], got[2], got[3]), cached):
        for fld in ("twb", "H", "edge_chi2", "outlier"):
            np.testing.assert_array_equal(getattr(g, fld), getattr(c, fld), err_msg=fld)
        assert (g.n_bad, g.n_inliers) == (c.n_bad, c.n_inliers)


def test_refusals(solver):
    import ctypes as C
    from orb_slam3_study_kr_amd import capi
    f = lc.frame("stereo-m0")
    p = f.as_struct()
    H, b = np.zeros((15, 15)), np.zeros(15)
    d = capi.c_double_p
    lib = solver.lib
    assert lib.osh_posei_linearize(solver.ctx, C.byref(p), None, capi.ptr(b, d)) == capi.OSH_ERR_INVALID
    assert lib.osh_posei_linearize(solver.ctx, C.byref(p), capi.ptr(H, d), None) == capi.OSH_ERR_INVALID
    assert lib.osh_posei_linearize(solver.ctx, None, capi.ptr(H, d), capi.ptr(b, d)) == capi.OSH_ERR_INVALID
    p.mode = 2
    assert lib.osh_posei_linearize(solver.ctx, C.byref(p), capi.ptr(H, d), capi.ptr(b, d)) == capi.OSH_ERR_INVALID
    p.mode = 0
    p.n_edges = -1
    assert lib.osh_posei_linearize(solver.ctx, C.byref(p), capi.ptr(H, d), capi.ptr(b, d)) == capi.OSH_ERR_INVALID
