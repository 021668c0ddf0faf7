"""The host build of csrc/two_view.h (TwoViewReconstruction, the monocular initialisation) through the test library, stage by stage
against the numpy restatement (tests/two_view_numpy.py): the models of every minimal set, the scores and inlier flags from the
build's own models, the RANSAC choice and the branch, CheckRT from the build's own (R, t), the decision tables on hand-written rows,
Normalize, and the minimal sets TwoViewReconstruction::Reconstruct draws."""
import ctypes as C
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import two_view_numpy as tv
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_two_view as st

F = np.float32
ROOT = Path(__file__).resolve().parent.parent
NAMES = list(st.CASES)
# what each named case ends as.  planar: with isotropic pixel noise every fundamental matrix of the family [e]x H fits the points of a
# plane, and its point-to-line distances are never larger than the homography's point-to-point ones, so SH stays just below SF
# (RH 0.49 here) and the reference's RH > 0.50 sends the case to ReconstructF, whose hypotheses a plane leaves short of points.
# coincident_accepted is the case that ReconstructH accepts: four distinct correspondences on a plane, 30 copies of each.
STATUS = {"coincident_accepted": capi.OSH_TWOVIEW_ACCEPTED_H, "general": capi.OSH_TWOVIEW_ACCEPTED_F, "planar": capi.OSH_TWOVIEW_TOO_FEW_POINTS, "rotation": capi.OSH_TWOVIEW_LOW_PARALLAX,
          "ambiguous": capi.OSH_TWOVIEW_NO_CLEAR_WINNER, "sparse": capi.OSH_TWOVIEW_TOO_FEW_POINTS}


@functools.lru_cache(maxsize=None)
def case(name, iterations=200):
    scene = st.make_scene(**st.CASES[name])
    pb = st.problem(scene, iterations)
    return scene, pb, orb.two_view_cpu([pb], debug=True)[0][0]


@pytest.mark.parametrize("name", NAMES)
def test_models_of_every_minimal_set(name):
    """The normalised model of every hypothesis against LAPACK's, sign fixed: each entry within one float32 step of the model's
    largest entry.  Hypotheses whose (sigma8 - sigma9) / sigma1 is below 1e-6 have no defined null vector and are left out, at most
    2 % of a case's per model; the `coincident` kind exists to be degenerate: finite output only."""
    _, pb, got = case(name)
    assert np.isfinite(got["debug_model_n"]).all() and np.isfinite(got["debug_score"]).all()
    if st.CASES[name]["kind"] == "coincident":
        return
    for model in (0, 1):
        left_out = 0
        for it in range(pb.n_iterations):
            A = tv.system(model, pb.pn1[pb.sets[it]], pb.pn2[pb.sets[it]])
            if tv.singular_gap(A) < 1e-6:
                left_out += 1
                continue
            exp = tv.fix_sign(tv.normalised_model(model, tv.null_vector(A)))
            mine = got["debug_model_n"][model, it]
            mine = tv.fix_sign(mine) if model == 0 else mine     # the rank-2 form has no sign freedom ...
            if model == 1 and np.abs(mine + exp).max() < np.abs(mine - exp).max():
                exp = -exp                                        # ... beyond the null vector's own
            step = np.spacing(np.abs(exp).max())
            assert np.abs(mine.astype(np.float64) - exp.astype(np.float64)).max() <= step, (name, model, it)
        assert left_out <= 0.02 * pb.n_iterations, (name, model, left_out)


@pytest.mark.parametrize("name", NAMES)
def test_transforms_scores_and_choice_from_the_builds_own_models(name):
    """Given the build's normalised models: the same final models, score bits and winner; RH and the branch; the inlier flags."""
    _, pb, got = case(name)
    scores = np.zeros((2, pb.n_iterations), F)
    for model in (0, 1):
        for it in range(pb.n_iterations):
            M, Minv = tv.final_model(model, got["debug_model_n"][model, it], pb.T1, pb.T2)
            assert np.array_equal(tv.bits(M), tv.bits(got["debug_model"][model, it])), (name, model, it)
            scores[model, it] = tv.check(model, M, Minv, pb.sigma, pb.pt1, pb.pt2)[0]
        assert np.array_equal(tv.bits(scores[model]), tv.bits(got["debug_score"][model])), (name, model)
    (sh, ih), (sf, i_f) = tv.select(scores[0]), tv.select(scores[1])
    assert (ih, i_f) == (int(got["best_h"][0]), int(got["best_f"][0]))
    assert tv.bits(sh) == tv.bits(got["sh"])[0] and tv.bits(sf) == tv.bits(got["sf"])[0]
    br, _ = tv.branch(sh, sf)
    assert br == got["info"][0]
    if br >= 0:
        model, it = (0, ih) if br == 1 else (1, i_f)
        M, Minv = tv.final_model(model, got["debug_model_n"][model, it], pb.T1, pb.T2)
        assert np.array_equal(tv.bits(M), tv.bits(got["H21" if br == 1 else "F21"]))
        _, inl, _ = tv.check(model, M, Minv, pb.sigma, pb.pt1, pb.pt2)
        assert np.array_equal(inl, got["inlier"].astype(bool)) and int(inl.sum()) == got["info"][1]


@pytest.mark.parametrize("name", NAMES)
def test_check_rt_from_the_builds_own_motion_hypotheses(name):
    """nGood of every hypothesis away from the thresholds, the winner's flags and points, the parallax bits from the kept cosines."""
    _, pb, got = case(name)
    n_hyp, winner = int(got["info"][2]), int(got["info"][3])
    assert n_hyp == (8 if got["info"][0] == 1 else 4)
    inl = got["inlier"].astype(bool)
    for hyp in range(n_hyp):
        e = tv.check_rt(pb.K, got["debug_R"][hyp], got["debug_t"][hyp], pb.sigma, pb.pt1, pb.pt2, inl)
        assert abs(e["n_good"] - int(got["n_good"][hyp])) <= int(e["borderline"].sum()), (name, hyp)
        if hyp != winner:
            continue
        code = np.where(got["x3d"].any(axis=1), np.where(got["triangulated"] == 1, 2, 1), 0)
        firm = ~e["borderline"]
        assert np.array_equal(code[firm], e["code"][firm]), name
        both = (code > 0) & (e["code"] > 0)
        if both.any():
            assert tv.ulp_distance(got["x3d"][both], e["x3d"][both]).max() <= 1, name
        # the same cosines kept: the build's points in place of the triangulation
        same = tv.check_rt(pb.K, got["debug_R"][hyp], got["debug_t"][hyp], pb.sigma, pb.pt1, pb.pt2, inl, x3d=got["x3d"])
        kept = same["cos"][code > 0]
        assert int(got["n_good"][hyp]) == kept.shape[0]
        assert tv.bits(tv.parallax_of(kept)) == tv.bits(got["parallax"])[hyp], name
    assert not got["n_good"][n_hyp:].any() and not got["parallax"][n_hyp:].any()
    status, w = tv.decide(int(got["info"][0]), int(got["info"][1]), got["n_good"], got["parallax"])
    assert (status, w) == (int(got["status"][0]), winner)
    if winner >= 0:
        assert np.array_equal(got["T21"][:9], got["debug_R"][winner].reshape(9)) and np.array_equal(got["T21"][9:], got["debug_t"][winner])


@pytest.mark.parametrize("name", sorted(STATUS))
def test_named_cases_end_as_stated(name):
    scene, _, got = case(name)
    assert int(got["status"][0]) == STATUS[name]
    if name == "general":
        rot, tdir = tv.truth_error(got["T21"], scene.R, scene.t)
        assert rot < 1.0 and tdir < 3.0, (rot, tdir)      # a quarter pixel of noise at f = 500 is 0.03 degrees per ray
    if name == "coincident_accepted":
        # the H branch, 8 hypotheses, all 120 matches inliers and counted by the winner; noise-free pixels rounded to float32
        assert got["info"][0] == 1 and got["info"][2] == 8 and got["info"][1] == 120 and got["n_good"][got["info"][3]] == 120
        rot, tdir = tv.truth_error(got["T21"], scene.R, scene.t)
        assert rot < 0.01 and tdir < 0.05, (rot, tdir)      # as test_motion_hypotheses_hold_the_truth: float32 behind a decomposition


def test_coincident_points_give_finite_output():
    _, pb, got = case("coincident")
    for k in ("T21", "sh", "sf", "H21", "F21", "x3d", "parallax", "debug_model", "debug_R", "debug_t"):
        assert np.isfinite(got[k]).all(), k
    assert got["info"][0] == 1          # the ReconstructH branch, as coincident_accepted


def _decide(branch, N, n_good, parallax):
    lib = capi.load_host_library()
    g = np.zeros(8, np.int32); g[:len(n_good)] = n_good
    p = np.zeros(8, F); p[:len(parallax)] = parallax
    w = C.c_int32(-7)
    status = lib.osh_host_two_view_decide(branch, N, capi.ptr(g, capi.c_int32_p), capi.ptr(p, capi.c_float_p), C.byref(w))
    assert (status, w.value) == tv.decide(branch, N, g, p), (branch, N, n_good, parallax)
    return status, w.value


def test_decision_table_of_reconstruct_f():
    A, W, T, L = capi.OSH_TWOVIEW_ACCEPTED_F, capi.OSH_TWOVIEW_NO_CLEAR_WINNER, capi.OSH_TWOVIEW_TOO_FEW_POINTS, capi.OSH_TWOVIEW_LOW_PARALLAX
    par = [2.0, 2.0, 2.0, 2.0]
    # nMinGood = max(int(0.9 * N), 50): N = 100 -> 90; N = 40 -> 50
    assert _decide(0, 100, [90, 0, 0, 0], par) == (A, 0)
    assert _decide(0, 100, [89, 0, 0, 0], par) == (T, 0)
    assert _decide(0, 40, [50, 0, 0, 0], par) == (A, 0)
    assert _decide(0, 40, [49, 0, 0, 0], par) == (T, 0)
    # nGood > 0.7 * maxGood: maxGood = 100 -> 70 is not similar, 71 is
    assert _decide(0, 100, [0, 100, 70, 0], par) == (A, 1)
    assert _decide(0, 100, [0, 100, 71, 0], par) == (W, 1)
    # ties: the first of the equal ones is the winner, and both are similar
    assert _decide(0, 100, [0, 95, 0, 95], par) == (W, 1)
    # parallax > minParallax, strictly
    assert _decide(0, 100, [0, 0, 0, 95], [9, 9, 9, 1.0]) == (L, 3)
    assert _decide(0, 100, [0, 0, 0, 95], [0, 0, 0, np.nextafter(F(1), F(2))]) == (A, 3)
    assert _decide(0, 100, [0, 0, 0, 0], par) == (T, 0)


def test_decision_table_of_reconstruct_h():
    A, W, T, L = capi.OSH_TWOVIEW_ACCEPTED_H, capi.OSH_TWOVIEW_NO_CLEAR_WINNER, capi.OSH_TWOVIEW_TOO_FEW_POINTS, capi.OSH_TWOVIEW_LOW_PARALLAX
    par = [2.0] * 8
    # secondBestGood < 0.75 * bestGood: best 100 -> 74 passes, 75 does not
    assert _decide(1, 100, [0, 0, 100, 74, 0, 0, 0, 0], par) == (A, 2)
    assert _decide(1, 100, [0, 0, 100, 75, 0, 0, 0, 0], par) == (W, 2)
    assert _decide(1, 100, [74, 0, 0, 0, 0, 0, 0, 100], par) == (A, 7)       # the earlier best becomes the second best
    assert _decide(1, 100, [100, 0, 0, 0, 100, 0, 0, 0], par) == (W, 0)      # a tie: the first stays the best
    # bestGood > minTriangulated (50), strictly
    assert _decide(1, 40, [51, 0, 0, 0, 0, 0, 0, 0], par) == (A, 0)
    assert _decide(1, 40, [50, 0, 0, 0, 0, 0, 0, 0], par) == (T, 0)
    # bestGood > 0.9 * N, strictly: N = 100 -> 91 passes, 90 does not
    assert _decide(1, 100, [0, 91, 0, 0, 0, 0, 0, 0], par) == (A, 1)
    assert _decide(1, 100, [0, 90, 0, 0, 0, 0, 0, 0], par) == (T, 1)
    # bestParallax >= minParallax
    assert _decide(1, 100, [0, 95, 0, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0, 0, 0]) == (A, 1)
    assert _decide(1, 100, [0, 95, 0, 0, 0, 0, 0, 0], [0, np.nextafter(F(1), F(0)), 0, 0, 0, 0, 0, 0]) == (L, 1)
    assert _decide(1, 100, [0] * 8, par) == (W, -1)


def _motion(branch, model, K):
    lib = capi.load_host_library()
    model, K = np.ascontiguousarray(model, F).reshape(9), np.ascontiguousarray(K, F).reshape(9)
    R, t = np.zeros((8, 3, 3), F), np.zeros((8, 3), F)
    n = lib.osh_host_two_view_motion(branch, capi.ptr(model, capi.c_float_p), capi.ptr(K, capi.c_float_p), capi.ptr(R, capi.c_float_p), capi.ptr(t, capi.c_float_p))
    return n, R, t


def test_motion_hypotheses_hold_the_truth():
    """The exact homography of the planar scene's plane and the exact fundamental matrix of the general scene, rounded to float32:
    one of the 8 / 4 motion hypotheses is the generator's (R, t) (rotation within 0.01 degrees, translation direction within 0.05:
    float32 matrices of condition about 1e3 behind the decomposition), every R is a rotation, and CheckRT of that hypothesis counts
    the scene's inliers and more than any other.  This is the one check of ReconstructH's geometry against a truth: no synthetic
    plane with isotropic noise reaches it through RH > 0.50 (see STATUS above)."""
    planar, general = case("planar")[0], case("general")[0]
    K = planar.K.astype(np.float64)
    n_pl, d = np.array([-0.35, 0.2, 1.0]), 5.0                      # the plane z = 5 + 0.35 x - 0.2 y as n . X = d
    H = K @ (planar.R + np.outer(planar.t, n_pl) / d) @ np.linalg.inv(K)
    tx = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    Kg = general.K.astype(np.float64)
    Fm = np.linalg.inv(Kg).T @ tx(general.t) @ general.R @ np.linalg.inv(Kg)
    for branch, model, scene, name in ((1, H / np.abs(H).max(), planar, "planar"), (0, Fm / np.abs(Fm).max(), general, "general")):
        n, R, t = _motion(branch, model, scene.K)
        assert n == (8 if branch else 4)
        errs = [tv.truth_error(np.concatenate([R[i].reshape(9), t[i]]), scene.R, scene.t) for i in range(n)]
        best = int(np.argmin([a + b for a, b in errs]))
        assert errs[best][0] < 0.01 and errs[best][1] < 0.05, (name, errs)
        for i in range(n):
            assert np.abs(R[i].astype(np.float64) @ R[i].astype(np.float64).T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(R[i].astype(np.float64)) - 1) < 1e-5
            assert abs(float(np.linalg.norm(t[i].astype(np.float64))) - 1) < 1e-6
        pb = case(name)[1]
        exact = np.abs(np.linalg.norm(pb.pt2.astype(np.float64) - _transfer(scene, pb), axis=1)) < 2.0   # the matches that are no outliers
        goods = [tv.check_rt(pb.K, R[i], t[i], pb.sigma, pb.pt1, pb.pt2, exact)["n_good"] for i in range(n)]
        assert goods[best] > 0.95 * exact.sum() and goods[best] == max(goods), (name, goods)
        status, winner = tv.decide(branch, int(exact.sum()), np.array(goods + [0] * (8 - n)), np.full(8, 5.0, F))
        assert winner == best
        # the plane of this scene leaves Faugeras' second solution in front of both cameras too (264 of 275 points), which is
        # ReconstructH's "no clear winner" even from the exact homography
        assert status == (capi.OSH_TWOVIEW_NO_CLEAR_WINNER if branch else capi.OSH_TWOVIEW_ACCEPTED_F), (name, goods)


def _transfer(scene, pb):
    """Where the first frame's matched pixels land in the second frame under the scene's true geometry (its plane for `planar`;
    for `general` the second frame's own pixel moved onto the epipolar line, which is what an inlier is there)."""
    K = scene.K.astype(np.float64)
    p1 = np.concatenate([pb.pt1.astype(np.float64), np.ones((pb.n, 1))], 1)
    if scene.name == "planar":
        H = K @ (scene.R + np.outer(scene.t, [-0.35, 0.2, 1.0]) / 5.0) @ np.linalg.inv(K)
        q = p1 @ H.T
        return q[:, :2] / q[:, 2:3]
    tx = np.array([[0, -scene.t[2], scene.t[1]], [scene.t[2], 0, -scene.t[0]], [-scene.t[1], scene.t[0], 0]])
    Fm = np.linalg.inv(K).T @ tx @ scene.R @ np.linalg.inv(K)
    line = p1 @ Fm.T
    p2 = pb.pt2.astype(np.float64)
    dist = (line[:, 0] * p2[:, 0] + line[:, 1] * p2[:, 1] + line[:, 2]) / np.hypot(line[:, 0], line[:, 1])
    return p2 - dist[:, None] * line[:, :2] / np.hypot(line[:, 0], line[:, 1])[:, None]


def test_normalize_equals_the_generators():
    """synth_two_view.normalize (what the problems carry) has the bits of the header's Normalize, over all keypoints."""
    lib = capi.load_host_library()
    scene = case("general")[0]
    for xy in (scene.keys1, scene.keys2, scene.keys1[:2], scene.keys2[:9]):
        xy = np.ascontiguousarray(xy, F)
        pn, T = np.zeros_like(xy), np.zeros(9, F)
        assert lib.osh_host_two_view_normalize(xy.shape[0], capi.ptr(xy, capi.c_float_p), capi.ptr(pn, capi.c_float_p), capi.ptr(T, capi.c_float_p)) == 0
        epn, eT = st.normalize(xy)
        assert np.array_equal(tv.bits(pn), tv.bits(epn)) and np.array_equal(tv.bits(T), tv.bits(eT.reshape(9)))


def test_sizes_around_a_wavefront_and_few_iterations():
    scene = case("general")[0]
    for n in (8, 9, 63, 64, 65):
        for it in (1, 3):
            pb = st.problem(scene, it, head=n)
            got = orb.two_view_cpu([pb], debug=True)[0][0]
            assert got["inlier"].shape == (n,) and got["debug_score"].shape == (2, it)
            for model in (0, 1):
                for k in range(it):
                    M, Minv = tv.final_model(model, got["debug_model_n"][model, k], pb.T1, pb.T2)
                    assert tv.bits(tv.check(model, M, Minv, pb.sigma, pb.pt1, pb.pt2)[0]) == tv.bits(got["debug_score"][model, k])
            if n == 8:
                assert (np.sort(pb.sets, axis=1) == np.arange(8)).all()
    empty = orb.two_view_cpu([st.problem(scene, 0, head=0), st.problem(scene, 0)])[0]
    assert [int(o["status"][0]) for o in empty] == [capi.OSH_TWOVIEW_NO_MODEL] * 2 and not empty[1]["inlier"].any()


_SETS_SCRIPT = """
import sys
import numpy as np
sys.path.insert(0, {tests!r})
import two_view_numpy as tv
from orb_slam3_study_kr_amd import host
from orb_slam3_study_kr_amd import synth_two_view as st
scene = st.make_scene(**st.CASES["general"])
n = int((scene.matches12 >= 0).sum())
stream = tv.glibc_rand(0, 2 * 200 * 8)
first = host.two_view_reconstruct(scene)
exp, used = tv.replay_sets(stream, n, 200)
assert np.array_equal(first["sets"], exp), "first call"
second = host.two_view_reconstruct(scene)
exp2, _ = tv.replay_sets(stream[used:], n, 200)
assert np.array_equal(second["sets"], exp2), "second call continues the stream"
assert not np.array_equal(first["sets"], second["sets"])
print("sets ok", first["info"][1])
"""


def test_reconstruct_draws_the_references_sets():
    """mvSets through TwoViewReconstruction::Reconstruct in a fresh process: the first call equals a replay of glibc's rand() seeded
    with 0, the second continues the stream without reseeding.  Without a device the class answers through the host build."""
    out = subprocess.run([sys.executable, "-c", _SETS_SCRIPT.format(tests=str(ROOT / "tests"))], cwd=ROOT, env=dict(os.environ),
                         capture_output=True, text=True)
    assert out.returncode == 0 and "sets ok" in out.stdout, out.stdout + out.stderr


def test_reconstruct_refuses_what_the_entry_refuses_with_or_without_a_device():
    """A non-finite keypoint among the matched ones: Reconstruct returns false before it chooses between device and host, and
    leaves vP3D and vbTriangulated as passed."""
    import dataclasses
    from orb_slam3_study_kr_amd import host
    scene = case("general")[0]
    keys2 = scene.keys2.copy()
    keys2[scene.matches12[scene.matches12 >= 0][3], 1] = np.nan
    got = host.two_view_reconstruct(dataclasses.replace(scene, keys2=keys2), p3d_in=np.full((5, 3), 7.5, F))
    assert not got["ok"] and got["info"][1] == 0 and got["n_p3d"] == 5 and got["n_triangulated"] == 0


def test_reconstruct_answers_beyond_the_device_limits():
    """More matches than OSH_TWOVIEW_MAX_MATCHES: Reconstruct runs the host build and says so on stderr; accepted by F here, with
    vP3D and vbTriangulated scattered into vKeys1 order."""
    from orb_slam3_study_kr_amd import host
    scene = st.make_scene(kind="general", seed=1, n=capi.OSH_TWOVIEW_MAX_MATCHES + 1, extra=3)
    got = host.two_view_reconstruct(scene, iterations=4)
    assert got["info"][1] == 0 and got["info"][2] == 4
    assert got["ok"] == (got["info"][0] in (capi.OSH_TWOVIEW_ACCEPTED_H, capi.OSH_TWOVIEW_ACCEPTED_F))
    pb = st.problem(scene, 4, sets=got["sets"])
    cpu = orb.two_view_cpu([pb])[0][0]
    assert int(cpu["status"][0]) == got["info"][0]
    if got["ok"] and got["info"][0] == capi.OSH_TWOVIEW_ACCEPTED_F:
        assert got["n_p3d"] == scene.keys1.shape[0] and got["n_triangulated"] == scene.keys1.shape[0]
        assert np.array_equal(tv.bits(got["p3d"][pb.idx1]), tv.bits(cpu["x3d"]))
        assert np.array_equal(got["triangulated"][pb.idx1], cpu["triangulated"])
        unmatched = scene.matches12 < 0
        assert not got["p3d"][unmatched].any() and not got["triangulated"][unmatched].any()


def test_refusals_need_no_device():
    """osh_orb_two_view_reconstruct looks at the problems before it asks for a context: with a null context every refusal comes
    back with its return code and its message, entry and problem named."""
    import dataclasses
    lib = capi.load_library()
    scene = case("general")[0]
    pb = st.problem(scene, 3, head=65)
    repeats = pb.sets.copy(); repeats[1, 7] = repeats[1, 0]
    outside = pb.sets.copy(); outside[2, 0] = 65
    seven = st.problem(scene, 1, head=7, sets=np.tile(np.arange(8, dtype=np.int32) % 7, (1, 1)))
    bad = [(dataclasses.replace(pb, sets=repeats), "osh_orb_two_view_reconstruct: problem 1: set 1 repeats index", capi.OSH_ERR_INVALID),
           (dataclasses.replace(pb, sets=outside), "osh_orb_two_view_reconstruct: problem 1: set 2: index 65 outside [0, 65)", capi.OSH_ERR_INVALID),
           (seven, "osh_orb_two_view_reconstruct: problem 1: 7 matches cannot fill a minimal set of 8", capi.OSH_ERR_INVALID)]
    for problem, message, code in bad:
        cp, cr, _keep, _outs = orb.two_view_args([pb, problem])
        assert lib.osh_orb_two_view_reconstruct(None, 2, cp, cr) == code
        assert message in capi.last_error(lib)
    cp, cr, _keep, _outs = orb.two_view_args([pb, pb])
    cp[1].sets = None
    assert lib.osh_orb_two_view_reconstruct(None, 2, cp, cr) == capi.OSH_ERR_INVALID
    assert "osh_orb_two_view_reconstruct: problem 1: NULL sets with n_iterations = 3" in capi.last_error(lib)
    few = st.problem(scene, 0, head=8)
    cp, cr, _keep, _outs = orb.two_view_args([few] * (capi.OSH_TWOVIEW_MAX_PROBLEMS + 1))
    assert lib.osh_orb_two_view_reconstruct(None, capi.OSH_TWOVIEW_MAX_PROBLEMS + 1, cp, cr) == capi.OSH_ERR_UNSUPPORTED
    assert "osh_orb_two_view_reconstruct: more than 4096 problems" in capi.last_error(lib)
    # what is valid gets as far as the context
    cp, cr, _keep, _outs = orb.two_view_args([pb])
    assert lib.osh_orb_two_view_reconstruct(None, 1, cp, cr) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
