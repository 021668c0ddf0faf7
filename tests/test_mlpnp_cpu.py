"""The host build of csrc/mlpnp.h (the statements osh_orb_mlpnp_solve runs on the device) against the numpy restatement of
MLPnPsolver (tests/mlpnp_numpy.py), stage by stage: the null-space projector, the rank decision, the null vector, computePose, a
Gauss-Newton step and every exit of mlpnp_gn, CheckInliers bit for bit, SetRansacParameters, and the record / Refine decision from
synthetic counts; and the measured spreads the device bound of mlpnp_cases.py comes from."""
import numpy as np
import pytest

import mlpnp_cases as mc
import mlpnp_numpy as mn
from orb_slam3_study_kr_amd import orb
from orb_slam3_study_kr_amd import synth_mlpnp as sm

EPS = np.finfo(np.float64).eps


def clean_scene(n=40, camera=sm.PINHOLE, seed=5):
    """No outliers, no noise, exact bearing vectors."""
    return sm.make_problem(seed=seed, n=n, iterations=0, camera_type=camera, noise_px=0.0, outlier_share=0.0, exact_bearing=True)


def true_x(pb):
    return np.concatenate([mn.rot2rodrigues(pb.pose[:9].reshape(3, 3)), pb.pose[9:]])


# ------------------------------------------------------------------------------------------------------------ stages
def test_nullspace_projector():
    rng = np.random.RandomState(1)
    fs = [np.array([0.3, -0.2, 1.0]), np.array([-0.4, 0.1, 1.0]), np.array([0.0, 0.0, 1.0]), np.array([-1e-9, 0.5, 1.0])] + list(rng.normal(0, 1, (20, 3)))
    for f in fs:
        N = orb.mlpnp_stage("nullspace", f)
        # three rounding steps per entry of N, two products and a sum per entry of N N^T: 16 eps covers both
        assert np.abs(N @ N.T - mn.projector(f)).max() <= 16 * EPS
        assert np.abs(N.T @ N - np.eye(2)).max() <= 16 * EPS
        assert np.abs(N.T @ f).max() <= 16 * EPS * np.linalg.norm(f)
        Nn = mn.nullspace(f)
        assert np.abs(Nn @ Nn.T - N @ N.T).max() <= 16 * EPS


def test_rank_decision():
    rng = np.random.RandomState(2)
    general = rng.normal(0, 1, (6, 3))
    plane0 = general.copy(); plane0[:, 2] = 0.0
    plane1 = general.copy(); plane1[:, 2] = 1.0
    tilted = plane0 @ sm.rodrigues([0.3, -0.2, 0.1]).T           # a plane through the origin, not axis-aligned: rank 2 only up to rounding
    line = np.outer(np.arange(1.0, 7.0), [0.5, -1.0, 2.0])
    for pts, want in ((general, 3), (plane0, 2), (plane1, 3), (line, 1), (np.zeros((6, 3)), 0)):
        S = pts.T @ pts
        assert orb.mlpnp_stage("rank", S) == want == mn.rank3(S)
        if want:
            assert np.linalg.matrix_rank(S) == want
    assert orb.mlpnp_stage("rank", tilted.T @ tilted) == mn.rank3(tilted.T @ tilted)


@pytest.mark.parametrize("kind", ("pinhole", "kb8", "planar"))
def test_null_vector_up_to_sign(kind):
    pb = mc.scene(kind)
    for idx in list(pb.sets[:4]) + [np.flatnonzero(pb.inlier)]:
        st = {}
        mn.compute_pose(pb.bearing[idx], pb.p3d[idx], stages=st)
        f, p = pb.bearing[idx], pb.p3d[idx]
        if st["planar"]:
            _, vecs = np.linalg.eigh(p.T @ p)
            p = p @ vecs
            cols = [(0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (2, 2), (0, 3), (1, 3), (2, 3)]
        else:
            cols = [(r, a) for r in range(3) for a in range(3)] + [(r, 3) for r in range(3)]
        ph = np.concatenate([p, np.ones((len(idx), 1))], 1)
        A = np.stack([(st["Ns"][:, r, :] * ph[:, a, None]).reshape(-1) for r, a in cols], 1)
        M = A.T @ A
        h = orb.mlpnp_stage("null_vector", M)
        ref = mn.null_vector(M)
        s = np.linalg.svd(M, compute_uv=False)
        # a singular vector moves by the perturbation over the gap to its neighbour: eps * s_max / s[-2], 64 for the accumulated sweeps
        bound = 64 * EPS * s[0] / s[-2]
        assert min(np.abs(h - ref).max(), np.abs(h + ref).max()) <= bound, (kind, len(idx))
        assert abs(np.linalg.norm(h) - 1) <= 64 * EPS


def test_numpy_jacobian_against_central_differences():
    pb = clean_scene()
    Ns = np.stack([mn.nullspace(f) for f in pb.bearing])
    x = true_x(pb) + np.array([0.2, -0.1, 0.15, 0.3, -0.2, 0.4])
    _, J = mn.residuals_and_jacs(x, pb.p3d, Ns)
    h = 1e-6
    for a in range(6):
        d = np.zeros(6); d[a] = h
        num = (mn.residuals(x + d, pb.p3d, Ns) - mn.residuals(x - d, pb.p3d, Ns)) / (2 * h)
        assert np.abs(num - J[:, :, a]).max() <= 1e-8   # h^2 truncation (1e-12) and eps / h rounding (2e-10), with room


def test_one_gauss_newton_step():
    for camera in (sm.PINHOLE, sm.KB8):
        pb = clean_scene(camera=camera)
        Ns = np.stack([mn.nullspace(f) for f in pb.bearing])
        x0 = true_x(pb) + np.array([0.05, -0.03, 0.04, 0.1, -0.2, 0.15])
        x, info = orb.mlpnp_stage("gauss_newton", pb.bearing, pb.p3d, x0, 1)
        ref, updates, reason = mn.gauss_newton(x0, pb.p3d, Ns, 1)
        assert list(info) == [updates, reason] == [1, 0]
        # the 6x6 system has a condition number below 1e5 here: eps * 1e5 on values of order 1, with room
        assert np.linalg.cond(sum(j.T @ j for j in mn.residuals_and_jacs(x0, pb.p3d, Ns)[1])) < 1e5
        assert np.abs(x - ref).max() <= 1e-10


def test_every_exit_of_the_gauss_newton():
    pb = clean_scene()
    Ns = np.stack([mn.nullspace(f) for f in pb.bearing])
    xt = true_x(pb)

    def both(x0, iterations=5):
        x, info = orb.mlpnp_stage("gauss_newton", pb.bearing, pb.p3d, x0, iterations)
        ref, updates, reason = mn.gauss_newton(x0, pb.p3d, Ns, iterations)
        assert list(info) == [updates, reason]
        return x, updates, reason

    def first_dx(x0):
        r, J = mn.residuals_and_jacs(x0, pb.p3d, Ns)
        Jm = J.reshape(-1, 6)
        return np.abs(np.linalg.solve(Jm.T @ Jm, Jm.T @ r.reshape(-1)))

    # the stop of :748: from the solution the first update is below 1e-5 everywhere; the update is applied
    x, updates, reason = both(xt)
    assert (updates, reason) == (1, 2)
    # converging from nearby: the stop after a few updates, at the solution
    x, updates, reason = both(xt + np.array([0.01, 0, 0, 0, 0.02, 0]))
    assert reason == 2 and 2 <= updates <= 5 and np.abs(x - xt).max() <= 1e-9
    # the break of :744 by max|dx| > 5: no update
    x0 = xt + np.array([0, 0, 0, 20.0, 0, 0])
    assert first_dx(x0).max() > 5
    x, updates, reason = both(x0)
    assert (updates, reason) == (0, 1) and np.array_equal(x, x0)
    # the break of :744 by min|dx| > 1 with max|dx| <= 5
    x0 = xt + np.array([-1.22, -1.528, 0.644, -2.836, 3.76, 3.409])
    dx = first_dx(x0)
    assert dx.min() > 1 and dx.max() <= 5
    x, updates, reason = both(x0)
    assert (updates, reason) == (0, 1) and np.array_equal(x, x0)
    # the bound: a NaN makes every comparison false, the loop runs its five rounds
    x0 = xt.copy(); x0[4] = np.nan
    x, updates, reason = both(x0)
    assert (updates, reason) == (5, 0) and np.isnan(x).all()
    # the bound of a shorter loop
    assert both(xt + np.array([0.3, -0.2, 0.1, 0.5, 0.5, -0.5]), 2)[1:] == (2, 0)


def test_plane_through_the_origin_goes_planar_and_the_same_plane_at_z_1_does_not():
    for z, want in ((0.0, 1), (1.0, 0)):
        pb = sm.make_problem(seed=11, n=60, iterations=4, plane_z=z, inlier_sets=True, noise_px=0.0)
        for idx in list(pb.sets) + [np.flatnonzero(pb.inlier)]:
            st = {}
            mn.compute_pose(pb.bearing[idx], pb.p3d[idx], stages=st)
            pose, info = orb.mlpnp_stage("compute_pose", pb.bearing[idx], pb.p3d[idx])
            assert info[0] == want == int(st["planar"])
    # the planar branch does not depend on the signs of the eigenvectors, which are free
    pb = mc.scene("planar")
    idx = pb.sets[0]
    ref = mn.compute_pose(pb.bearing[idx], pb.p3d[idx])
    for sign in ((-1, 1, 1), (1, -1, 1), (1, 1, -1), (-1, -1, -1)):
        rot, trans = mn.pose_difference(mn.compute_pose(pb.bearing[idx], pb.p3d[idx], eig_sign=sign), ref)
        assert rot <= 1e-9 and trans <= 1e-9


def host_poses():
    return [orb.mlpnp_stage("compute_pose", mc.scene(kind).bearing[idx], mc.scene(kind).p3d[idx])[0] for kind, _g, idx, _ref in mc.pose_cases()]


def test_measured_spreads():
    """computePose of the host build against numpy over the shared cases (minimal sets from inliers only, the refine of the true
    inlier set): the spreads written into mlpnp_cases.py still hold, and numpy against its np.longdouble Gauss-Newton beside them."""
    host = host_poses()
    extended = [mn.compute_pose(mc.scene(kind).bearing[idx], mc.scene(kind).p3d[idx], gn_dtype=np.longdouble) for kind, _g, idx, _ref in mc.pose_cases()]
    for group in ("general", "planar"):
        rot, trans = mc.spread(host, group)
        rl, tl = mc.spread(extended, group)
        print(f"{group}: host vs numpy {rot:.3e} rad {trans:.3e}; numpy vs longdouble {rl:.3e} rad {tl:.3e}")
        assert rot <= mc.HOST_VS_NUMPY[group][0] and trans <= mc.HOST_VS_NUMPY[group][1]
        assert rl <= mc.NUMPY_VS_LONGDOUBLE[group][0] and tl <= mc.NUMPY_VS_LONGDOUBLE[group][1]
    # the general cases end at the truth up to the pixel noise; the plane does not (the reference's planar scale)
    for (kind, group, idx, ref), pose in zip(mc.pose_cases(), host):
        if group == "general" and len(idx) > 6:
            rot, trans = mn.pose_difference(pose, mc.scene(kind).pose)
            assert rot <= 2e-3 and trans <= 1e-2


def test_numpy_error_against_truth():
    for camera in (sm.PINHOLE, sm.KB8):
        pb = mc.end_to_end(camera, 0.5)
        idx = np.flatnonzero(pb.inlier)
        rot, trans = mn.pose_difference(mn.compute_pose(pb.bearing[idx], pb.p3d[idx]), pb.pose)
        print(f"camera {camera}: numpy vs truth {rot:.3e} rad {trans:.3e}")
        assert rot <= mc.NUMPY_VS_TRUTH[camera][0] and trans <= mc.NUMPY_VS_TRUTH[camera][1]
        assert rot >= 0.5 * mc.NUMPY_VS_TRUTH[camera][0] and trans >= 0.5 * mc.NUMPY_VS_TRUTH[camera][1]   # the constants are not loose


# ------------------------------------------------------------------------------------------------------------ CheckInliers
@pytest.mark.parametrize("n", (10, 11, 63, 64, 65, 300))
def test_check_inliers_pinhole_bit_for_bit(n):
    pb = sm.make_problem(seed=1 + n, n=n, iterations=1, outlier_share=0.3, min_inliers=6)
    rng = np.random.RandomState(n)
    poses = [pb.pose]
    for s in (1e-6, 1e-4, 2e-3, 1e-2, 1e-1, 1.0):
        R = sm.rodrigues(rng.normal(0, s, 3)) @ pb.pose[:9].reshape(3, 3)
        poses.append(np.concatenate([R.reshape(9), pb.pose[9:] + rng.normal(0, s, 3)]))
    nan = pb.pose.copy(); nan[3] = np.nan
    poses.append(nan)
    count, mask = orb.mlpnp_check_inliers_cpu(pb, np.stack(poses))
    flags = orb.mask_bits(mask, n)
    for k, pose in enumerate(poses):
        want = mn.check_inliers(pb.camera_type, pb.camera, pose, pb.p3d, pb.p2d, pb.max_error)
        assert np.array_equal(flags[k], want) and count[k] == want.sum(), f"pose {k}"
    assert count[0] == pb.inlier.sum() and count[-1] < count[0]


# ------------------------------------------------------------------------------------------------------------ SetRansacParameters
@pytest.mark.parametrize("n,want", [(9, (10, 1)), (10, (10, 1)), (11, (10, 4)), (20, (10, 35)), (300, (150, 35))])
def test_ransac_parameters_of_relocalisation(n, want):
    """SetRansacParameters(0.99, 10, 300, 6, 0.5, 5.991) as Tracking::Relocalization calls it.  N = 9: more inliers asked for than
    correspondences (iterate answers bNoMore); N = 10: every correspondence an inlier, one iteration; N = 11: epsilon rises to
    10 / 11, ceil(log(0.01) / log(1 - 0.751..)) = 4; N = 20 and 300: epsilon stays 0.5, ceil(log(0.01) / log(0.875)) = 35."""
    got = orb.mlpnp_stage("ransac_parameters", n, 0.99, 10, 300, 6, 0.5)
    assert got == want == mn.ransac_parameters(n, 0.99, 10, 300, 6, 0.5)
    if n == 9:
        assert got[0] > n


def test_ransac_parameters_of_the_constructor():
    for n in (0, 6, 19, 20, 21, 300, 2048):
        assert orb.mlpnp_stage("ransac_parameters", n, 0.99, 8, 300, 6, 0.4) == mn.ransac_parameters(n, 0.99, 8, 300, 6, 0.4)
    assert orb.mlpnp_stage("ransac_parameters", 300, 0.99, 8, 300, 6, 0.4) == (120, 70)


# ------------------------------------------------------------------------------------------------------------ the decision
def replay_both(count, min_inliers, best_in, ok_in, record_count):
    record, out = orb.mlpnp_stage("replay", count, min_inliers, best_in, ok_in, record_count)
    records, d = mn.replay(count, min_inliers, best_in, ok_in, record_count)
    assert list(record) == records
    got = dict(zip(("first_hit", "hit_record", "hit_count", "best_iteration", "best_count", "best_refine_ok", "n_records"), (int(v) for v in out)))
    assert got == {k: int(v) for k, v in d.items()}
    return got


def test_decision_from_synthetic_counts():
    # an early return at the first hit: iteration 2 is the first record whose Refine succeeds (12 > 10); what follows does not matter
    d = replay_both([3, 10, 11, 50, 9], 10, 0, 0, [10, 12, 60])
    assert d == dict(first_hit=2, hit_record=1, hit_count=12, best_iteration=2, best_count=11, best_refine_ok=1, n_records=3)
    # the Refine comparison is strict: a refined count equal to min_inliers is a failure, the run is exhausted with a best
    d = replay_both([10, 11, 12], 10, 0, 0, [10, 10, 10])
    assert d == dict(first_hit=-1, hit_record=-1, hit_count=0, best_iteration=2, best_count=12, best_refine_ok=0, n_records=3)
    # exhaustion without a best
    d = replay_both([0, 9, 5], 10, 0, 0, [0, 0, 0])
    assert d == dict(first_hit=-1, hit_record=-1, hit_count=0, best_iteration=-1, best_count=0, best_refine_ok=0, n_records=0)
    # a second call: the best on entry (40 inliers, its Refine succeeds) is not beaten; iteration 1 has enough inliers and is not a
    # record, so the cached Refine of the earlier best answers there
    d = replay_both([4, 20, 45], 10, 40, 1, [50, 0, 0])
    assert d == dict(first_hit=1, hit_record=-1, hit_count=0, best_iteration=-1, best_count=40, best_refine_ok=1, n_records=1)
    # the same with a failed cached Refine: no hit until the record at iteration 2, whose Refine succeeds
    d = replay_both([4, 20, 45], 10, 40, 0, [50, 0, 0])
    assert d == dict(first_hit=2, hit_record=0, hit_count=50, best_iteration=2, best_count=45, best_refine_ok=1, n_records=1)
    # a record whose Refine fails replaces a best whose Refine succeeded: the later non-record iteration is no hit
    d = replay_both([41, 20], 10, 40, 1, [9, 0])
    assert d == dict(first_hit=-1, hit_record=-1, hit_count=0, best_iteration=0, best_count=41, best_refine_ok=0, n_records=1)
    # no iterations
    d = replay_both([], 10, 7, 1, [])
    assert d == dict(first_hit=-1, hit_record=-1, hit_count=0, best_iteration=-1, best_count=7, best_refine_ok=1, n_records=0)


# ------------------------------------------------------------------------------------------------------------ the whole host build
@pytest.mark.parametrize("camera", (sm.PINHOLE, sm.KB8))
def test_host_build_end_to_end(camera):
    pb = mc.end_to_end(camera, 0.5)
    o = orb.mlpnp_cpu([pb], debug=True)[0][0]
    assert int(o["first_hit"][0]) >= 0
    assert np.array_equal(orb.mask_bits(o["hit_mask"], pb.n), pb.inlier)
    for k in range(pb.sets.shape[0]):
        flags = mn.check_inliers(pb.camera_type, pb.camera, o["debug_pose"][k], pb.p3d, pb.p2d, pb.max_error)
        if camera == sm.PINHOLE:
            assert int(flags.sum()) == o["debug_count"][k]
    idx = np.flatnonzero(orb.mask_bits(o["best_mask"], pb.n))
    rot, trans = mn.pose_difference(o["hit_pose"], mn.compute_pose(pb.bearing[idx], pb.p3d[idx]))
    assert rot <= mc.HOST_VS_NUMPY["general"][0] and trans <= mc.HOST_VS_NUMPY["general"][1]


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_need_no_device():
    """osh_orb_mlpnp_solve looks at the problems before it asks for a context: with a null context every refusal comes back with
    its return code and its message, the second problem named."""
    import dataclasses
    from orb_slam3_study_kr_amd import capi
    lib = capi.load_library()
    pb = sm.make_problem(seed=4, n=65, iterations=3)
    repeats = pb.sets.copy(); repeats[1, 5] = repeats[1, 0]
    outside = pb.sets.copy(); outside[2, 0] = 65
    five = dataclasses.replace(pb, bearing=pb.bearing[:5], p3d=pb.p3d[:5], p2d=pb.p2d[:5], max_error=pb.max_error[:5],
                               sets=np.tile(np.arange(6, dtype=np.int32) % 5, (1, 1)))
    bad = [(dataclasses.replace(pb, sets=repeats), "osh_orb_mlpnp_solve: problem 1: set 1 repeats index", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, sets=outside), "osh_orb_mlpnp_solve: problem 1: set 2: index 65 outside [0, 65)", capi.OSH_ERR_INVALID),
           (five, "osh_orb_mlpnp_solve: problem 1: 5 correspondences cannot fill a minimal set of 6", capi.OSH_ERR_INVALID)]
    for problem, message, code in bad:
        cp, cr, _keep, _outs = orb.mlpnp_args([pb, problem])
        assert lib.osh_orb_mlpnp_solve(None, 2, cp, cr) == code
        assert message in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.mlpnp_args([pb, pb])
    cp[1].sets = None
    assert lib.osh_orb_mlpnp_solve(None, 2, cp, cr) == capi.OSH_ERR_INVALID
    assert "osh_orb_mlpnp_solve: problem 1: NULL sets with n_iterations = 3" in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.mlpnp_args([pb] * (capi.OSH_MLPNP_MAX_PROBLEMS + 1))
    assert lib.osh_orb_mlpnp_solve(None, capi.OSH_MLPNP_MAX_PROBLEMS + 1, cp, cr) == capi.OSH_ERR_UNSUPPORTED
    assert "osh_orb_mlpnp_solve: more than 64 problems" in capi.last_error(lib)
    # what is valid gets as far as the context
    cp, cr, _keep, _outs = orb.mlpnp_args([pb])
    assert lib.osh_orb_mlpnp_solve(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
