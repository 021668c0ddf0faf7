"""osh_orb_two_view_reconstruct (TwoViewReconstruction, the monocular initialisation) on the device against the host build of
csrc/two_view.h: the named generator cases, match counts around a wavefront with 1, 3 and 200 iterations, a batch with an
empty-iteration problem in the middle, fully written results, refusals, the independence of a call from what its context ran before,
and the drop-in entry points (TwoViewReconstruction::Reconstruct, Pinhole / KannalaBrandt8::ReconstructWithTwoViews)."""
import dataclasses
import functools

import numpy as np
import pytest

import two_view_numpy as tv
from orb_slam3_study_kr_amd import capi, host, orb
from orb_slam3_study_kr_amd import synth_bow as sb
from orb_slam3_study_kr_amd import synth_newpoints as sn
from orb_slam3_study_kr_amd import synth_stereo as ss
from orb_slam3_study_kr_amd import synth_two_view as st

pytestmark = pytest.mark.gpu

F = np.float32
NAMES = list(st.CASES)
# see tests/test_two_view_cpu.py for why `planar` ends in ReconstructF
STATUS = {"coincident_accepted": capi.OSH_TWOVIEW_ACCEPTED_H, "general": capi.OSH_TWOVIEW_ACCEPTED_F, "planar": capi.OSH_TWOVIEW_TOO_FEW_POINTS, "rotation": capi.OSH_TWOVIEW_LOW_PARALLAX,
          "ambiguous": capi.OSH_TWOVIEW_NO_CLEAR_WINNER, "sparse": capi.OSH_TWOVIEW_TOO_FEW_POINTS}
EXACT = ("status", "best_h", "best_f", "info", "inlier", "triangulated", "n_good")
BITS = ("sh", "sf", "parallax", "H21", "F21")


@functools.lru_cache(maxsize=None)
def scene_of(name):
    return st.make_scene(**st.CASES[name])


@functools.lru_cache(maxsize=None)
def case(name, iterations=200, head=None):
    pb = st.problem(scene_of(name), iterations, head=head)
    return pb, orb.two_view_cpu([pb], debug=True)[0][0]


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


def assert_equals_host(got, cpu, what):
    """Status, winner indices, scores, flags, nGood and parallax bit for bit; T21 and x3D within one float32 step."""
    for k in EXACT:
        assert np.array_equal(got[k], cpu[k]), f"{what}: {k}: {got[k]} vs {cpu[k]}"
    for k in BITS:
        assert np.array_equal(tv.bits(got[k]), tv.bits(cpu[k])), f"{what}: {k}"
    assert tv.ulp_distance(got["T21"], cpu["T21"]).max() <= 1, what
    if got["x3d"].size:
        assert tv.ulp_distance(got["x3d"], cpu["x3d"]).max() <= 1, what
    for k in ("debug_model_n", "debug_model", "debug_score", "debug_R", "debug_t"):
        if k in got and k in cpu:
            assert np.array_equal(tv.bits(got[k]), tv.bits(cpu[k])), f"{what}: {k}"


def assert_same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k}"


@pytest.mark.parametrize("name", NAMES)
def test_named_cases_equal_the_host_build(matcher, name):
    pb, cpu = case(name)
    got = matcher.two_view_reconstruct([pb], debug=True)[0]
    assert_equals_host(got, cpu, name)
    if name in STATUS:
        assert int(got["status"][0]) == STATUS[name]
    if int(got["status"][0]) in (capi.OSH_TWOVIEW_ACCEPTED_H, capi.OSH_TWOVIEW_ACCEPTED_F):
        # against the generator's truth: the host build's own error plus one float32 step of an angle of that size in degrees
        sc = scene_of(name)
        (rot, tdir), (rot_cpu, tdir_cpu) = tv.truth_error(got["T21"], sc.R, sc.t), tv.truth_error(cpu["T21"], sc.R, sc.t)
        slack = float(np.degrees(np.spacing(F(1))))
        assert rot <= rot_cpu + slack and tdir <= tdir_cpu + slack, (rot, rot_cpu, tdir, tdir_cpu)


@pytest.mark.parametrize("iterations", [1, 3, 200])
@pytest.mark.parametrize("n", [8, 9, 63, 64, 65, 300])
def test_match_and_iteration_counts(matcher, n, iterations):
    pb, cpu = case("general", iterations, n)
    got = matcher.two_view_reconstruct([pb], debug=True)[0]
    assert got["inlier"].shape == (n,) and got["x3d"].shape == (n, 3) and got["debug_score"].shape == (2, iterations)
    assert_equals_host(got, cpu, f"{n} matches, {iterations} iterations")


def test_later_stages_from_the_devices_own_models_equal_the_restatement(matcher):
    """As the CPU test does for the host build: scores, choice and CheckRT in numpy from the device's debug models and (R, t)."""
    pb, _ = case("general")
    got = matcher.two_view_reconstruct([pb], debug=True)[0]
    for model in (0, 1):
        for it in range(0, pb.n_iterations, 7):
            M, Minv = tv.final_model(model, got["debug_model_n"][model, it], pb.T1, pb.T2)
            assert np.array_equal(tv.bits(M), tv.bits(got["debug_model"][model, it]))
            assert tv.bits(tv.check(model, M, Minv, pb.sigma, pb.pt1, pb.pt2)[0]) == tv.bits(got["debug_score"][model, it])
        best, idx = tv.select(got["debug_score"][model])
        assert idx == int(got["best_h" if model == 0 else "best_f"][0]) and tv.bits(best) == tv.bits(got["sh" if model == 0 else "sf"])[0]
    winner, inl = int(got["info"][3]), got["inlier"].astype(bool)
    for hyp in range(int(got["info"][2])):
        e = tv.check_rt(pb.K, got["debug_R"][hyp], got["debug_t"][hyp], pb.sigma, pb.pt1, pb.pt2, inl)
        assert abs(e["n_good"] - int(got["n_good"][hyp])) <= int(e["borderline"].sum())
    same = tv.check_rt(pb.K, got["debug_R"][winner], got["debug_t"][winner], pb.sigma, pb.pt1, pb.pt2, inl, x3d=got["x3d"])
    assert tv.bits(tv.parallax_of(same["cos"][got["x3d"].any(axis=1)])) == tv.bits(got["parallax"])[winner]


def test_batch_with_an_empty_problem_in_the_middle_equals_the_single_calls(matcher):
    a, b, c = case("general")[0], st.problem(scene_of("planar"), 0), case("coincident", 3)[0]
    batch = matcher.two_view_reconstruct([a, b, c], debug=True)
    assert [o["inlier"].shape[0] for o in batch] == [a.n, b.n, c.n]
    assert int(batch[1]["status"][0]) == capi.OSH_TWOVIEW_NO_MODEL and batch[1]["info"].tolist() == [-1, 0, 0, -1]
    for pb, got in zip((a, b, c), batch):
        assert_same(got, matcher.two_view_reconstruct([pb], debug=True)[0], pb.name)
    assert matcher.two_view_reconstruct([]) == []


def test_every_result_word_is_written(matcher):
    for pb in (case("general", 3, 65)[0], st.problem(scene_of("planar"), 0, head=0), case("coincident", 3)[0]):
        ref = matcher.two_view_reconstruct([pb], debug=True)[0]
        for fill in (0xAB, 0x5C):
            cp, cr, _keep, outs = orb.two_view_args([pb], debug=True, fill=fill)
            capi.check(matcher.lib.osh_orb_two_view_reconstruct(matcher.ctx, 1, cp, cr), "osh_orb_two_view_reconstruct", matcher.lib)
            assert_same(outs[0], ref, f"{pb.name} pre-filled with {fill:#x}")


def test_refused_calls_leave_the_context_usable(matcher):
    pb, cpu = case("general", 3, 65)
    before = matcher.two_view_reconstruct([pb], debug=True)[0]
    sets = pb.sets.copy(); sets[1, 5] = sets[1, 2]
    pixel = pb.pt2.copy(); pixel[7, 1] = np.inf
    bad = {"repeats index": dataclasses.replace(pb, sets=sets),
           "cannot fill a minimal set": st.problem(scene_of("general"), 3, head=7, sets=np.tile(np.arange(8, dtype=np.int32) % 7, (3, 1))),
           "coordinate not finite": dataclasses.replace(pb, pt2=pixel)}
    for message, problem in bad.items():
        with pytest.raises(capi.OshError, match=message) as err:
            matcher.two_view_reconstruct([pb, problem])
        assert err.value.code == capi.OSH_ERR_INVALID
        assert_same(matcher.two_view_reconstruct([pb], debug=True)[0], before, f"after '{message}'")
    assert_equals_host(before, cpu, "refusals")


def test_over_the_limit_is_unsupported_and_reconstruct_still_answers(matcher):
    scene = st.make_scene(kind="general", seed=1, n=capi.OSH_TWOVIEW_MAX_MATCHES + 1, extra=3)
    pb = st.problem(scene, 2)
    with pytest.raises(capi.OshError, match="more than 8192 matches") as err:
        matcher.two_view_reconstruct([pb])
    assert err.value.code == capi.OSH_ERR_UNSUPPORTED
    many = st.problem(scene_of("sparse"), capi.OSH_TWOVIEW_MAX_ITERATIONS + 1)
    with pytest.raises(capi.OshError, match="more than 1024 iterations") as err:
        matcher.two_view_reconstruct([many])
    assert err.value.code == capi.OSH_ERR_UNSUPPORTED
    got = host.two_view_reconstruct(scene, iterations=2)
    cpu = orb.two_view_cpu([st.problem(scene, 2, sets=got["sets"])])[0][0]
    assert got["info"][1] == 0 and got["info"][0] == int(cpu["status"][0])


def test_result_does_not_depend_on_what_the_context_ran_before(hip_lib, monkeypatch):
    """The stereo, new-point and bag-of-words entries between calls, in two orders, larger and smaller problems first: the same
    bits as on a fresh context."""
    monkeypatch.setenv("OSH_ZERO_NEW_BUFFERS", "1")
    big, small = [case("general")[0], case("rotation")[0]], [case("general", 3, 65)[0]]
    rect = [ss.make_stereo_frame(301, n_left=65, n_right=257, n_levels=3)]
    seg = [sn.make_segment(seed=3, kind="stereo", n=130)]
    tree = sb.make_vocab(41, k=10, L=4)
    desc = [np.random.default_rng(3).integers(0, 256, (200, 32), dtype=np.uint8)]
    with orb.BowVocab(tree) as vocab:
        others = {"stereo": lambda m: m.stereo_match(rect), "newpoints": lambda m: m.triangulate_new_points(seg),
                  "bow": lambda m: m.bow_transform(vocab, desc)}
        with orb.OrbMatcher(0) as fresh:
            ref_big = fresh.two_view_reconstruct(big, debug=True)
        with orb.OrbMatcher(0) as fresh:
            ref_small = fresh.two_view_reconstruct(small, debug=True)
        for order in (("stereo", "newpoints", "bow"), ("bow", "newpoints", "stereo")):
            with orb.OrbMatcher(0) as m:
                for k, other in enumerate(order):
                    others[other](m)
                    pbs, ref = (big, ref_big) if k % 2 == 0 else (small, ref_small)
                    for got, r, pb in zip(m.two_view_reconstruct(pbs, debug=True), ref, pbs):
                        assert_same(got, r, f"{pb.name} after {other} ({order})")
                for got, r in zip(m.two_view_reconstruct(small, debug=True), ref_small):
                    assert_same(got, r, "small after big")
                # without the debug arrays the per-iteration models stay in device work memory: the same results
                for got, r in zip(m.two_view_reconstruct(big), ref_big):
                    assert_same(got, {k: r[k] for k in got}, "without debug")


def test_times_are_zero_before_a_call_and_kept_under_profiling(hip_lib):
    pb, _ = case("general", 3, 65)
    with orb.OrbMatcher(0) as m:
        assert np.array_equal(m.two_view_times(), np.zeros(4))
        m.set_profiling(True)
        m.two_view_reconstruct([pb])
        t = m.two_view_times()
        assert (t >= 0).all() and t.sum() > 0


# ------------------------------------------------------------------------------------------ the drop-in entry points
def _c_abi_of(matcher, scene, sets):
    pb = st.problem(scene, sets.shape[0], sets=sets)
    return pb, matcher.two_view_reconstruct([pb])[0]


@pytest.mark.parametrize("camera", ["class", "pinhole"])
@pytest.mark.parametrize("name", ["general", "rotation", "coincident", "coincident_accepted"])
def test_reconstruct_through_the_class_equals_the_c_abi(matcher, name, camera):
    """The same problem (the sets the class drew) through the C-ABI: the status, T21 through the quaternion of Sophus::SE3f, and
    vP3D / vbTriangulated scattered into vKeys1 order; a call that returns false leaves all three as passed."""
    scene = scene_of(name)
    n1 = scene.keys1.shape[0]
    marker = np.full((5, 3), 7.5, F)
    got = host.two_view_reconstruct(scene, camera, p3d_in=marker)
    assert got["info"][1] == 1 and got["info"][2] == 200
    pb, ref = _c_abi_of(matcher, scene, got["sets"])
    status = int(ref["status"][0])
    assert got["info"][0] == status and got["ok"] == (status in (capi.OSH_TWOVIEW_ACCEPTED_H, capi.OSH_TWOVIEW_ACCEPTED_F))
    if name in ("general", "coincident_accepted"):        # accepted whichever sets the class drew (30 draws of each were)
        assert status == STATUS[name]
        cpu = orb.two_view_cpu([pb])[0][0]
        (rot, tdir), (rot_cpu, tdir_cpu) = tv.truth_error(ref["T21"], scene.R, scene.t), tv.truth_error(cpu["T21"], scene.R, scene.t)
        slack = float(np.degrees(np.spacing(F(1))))
        assert rot <= rot_cpu + slack and tdir <= tdir_cpu + slack, (rot, rot_cpu, tdir, tdir_cpu)
    if not got["ok"]:
        assert got["n_p3d"] == 5 and np.array_equal(got["p3d"][:5], marker) and got["n_triangulated"] == 0
        return
    assert np.abs(got["T21"] - ref["T21"]).max() <= 4 * np.spacing(F(1))      # matrix -> unit quaternion -> matrix
    assert got["n_triangulated"] == n1
    tri = np.zeros(n1, np.uint8); tri[pb.idx1] = ref["triangulated"]
    assert np.array_equal(got["triangulated"], tri)
    if status == capi.OSH_TWOVIEW_ACCEPTED_F:
        p3d = np.zeros((n1, 3), F); p3d[pb.idx1] = ref["x3d"]
        assert got["n_p3d"] == n1 and np.array_equal(tv.bits(got["p3d"]), tv.bits(p3d))
    else:                                                                     # ReconstructH does not assign vP3D (:725-731)
        assert got["n_p3d"] == 5 and np.array_equal(got["p3d"][:5], marker)
        assert ref["triangulated"].sum() >= 100 and ref["x3d"].any(axis=1).sum() >= 100   # while the C-ABI carries the points


def test_kannala_brandt_reconstructs_from_fisheye_pixels(matcher):
    """KannalaBrandt8::ReconstructWithTwoViews on the fisheye pixels of the general scene: the keypoints undistorted by unproject and
    K (restated through tests/fisheye_stereo_numpy.py), then the same Reconstruct: accepted, equal to the C-ABI call on the
    undistorted problem, and as close to the truth as the host build on it plus one float32 step."""
    import fisheye_stereo_numpy as fn
    scene = st.make_scene(**dict(st.CASES["general"], fisheye=True))
    got = host.two_view_reconstruct(scene, "kb8")
    assert got["ok"] and got["info"][1] == 1 and got["info"][0] == capi.OSH_TWOVIEW_ACCEPTED_F
    cam = scene.kb8

    def undistort(keys):
        out = np.zeros_like(keys)
        for i, (x, y) in enumerate(keys):
            rx, ry, _ = fn.unproject(cam, 1e-6, x, y)
            out[i] = F(F(cam[0] * rx) + cam[2]), F(F(cam[1] * ry) + cam[3])
        return out
    plain = dataclasses.replace(scene, keys1=undistort(scene.keys1), keys2=undistort(scene.keys2), kb8=None)
    pb, ref = _c_abi_of(matcher, plain, got["sets"])
    assert int(ref["status"][0]) == capi.OSH_TWOVIEW_ACCEPTED_F
    assert np.abs(got["T21"] - ref["T21"]).max() <= 4 * np.spacing(F(1))
    p3d = np.zeros((scene.keys1.shape[0], 3), F); p3d[pb.idx1] = ref["x3d"]
    assert np.array_equal(tv.bits(got["p3d"]), tv.bits(p3d))
    cpu = orb.two_view_cpu([pb])[0][0]
    (rot, tdir), (rot_cpu, tdir_cpu) = tv.truth_error(ref["T21"], scene.R, scene.t), tv.truth_error(cpu["T21"], scene.R, scene.t)
    slack = float(np.degrees(np.spacing(F(1))))
    assert rot <= rot_cpu + slack and tdir <= tdir_cpu + slack and rot_cpu < 1.0 and tdir_cpu < 3.0, (rot, rot_cpu, tdir, tdir_cpu)
