"""osh_orb_fuse_search (the search of ORBmatcher::Fuse for one map point list and many target keyframes) on the device against the
numpy restatement (tests/fuse_numpy.py) and the header's host build (csrc/orb_fuse.h), bit for bit on every output."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

import fuse_class_cases as fc
import fuse_numpy as fn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_bow as sb
from orb_slam3_study_kr_amd import synth_fast as sfa
from orb_slam3_study_kr_amd import synth_stereo as ss

pytestmark = pytest.mark.gpu

CAMERAS = sorted(fn.CAMERAS)
MODES = [fn.CHI2, fn.SIM3]


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


def assert_three_way(matcher, targets, pts, mode, exp, what):
    got = matcher.fuse_search(targets, pts, mode)
    assert fn.same_bits(got, exp) == [], what
    assert fn.same_bits(got, orb.fuse_cpu(targets, pts, mode)[0]) == [], what
    return got


@pytest.mark.parametrize("mode", MODES, ids=["chi2", "sim3"])
@pytest.mark.parametrize("camera", CAMERAS)
def test_cameras_and_modes_equal_the_restatement_and_the_host_build(matcher, camera, mode):
    """K = 8, P = 300: targets of 200, 0 and 1 keypoints, one that no point passes, a window of more than 64 cells, cells of 70 and
    of OSH_FUSE_MAX_CELL_ENTRIES entries, null entries in the list."""
    targets, pts, exp = fn.shape_case(camera, mode)
    got = assert_three_way(matcher, targets, pts, mode, exp, (camera, mode))
    st = got["stage"]
    assert [t.n_keys for t in targets[:3]] == [200, 0, 1]
    assert not (st[3] >= fn.EMPTY).any() and not (st[1] == fn.SEARCHED).any()          # nothing passes target 3; target 1 has no keypoint
    assert all((st == s).any() for s in range(7))                                     # every exit is taken
    assert (got["best_idx"][st == fn.SEARCHED] >= 0).sum() >= 100 and (got["n_candidates"] >= 2).sum() >= 20
    big = targets[4]                                                                   # th = 40: 2 * 40 * 1.2^level / 10 cells a side
    assert (got["radius"][4] > 40).any() and big.th == 40.0
    # the clustered cells (70 and 255 entries) are walked to their end: pairs whose window holds them count what the restatement counts,
    # and in every parametrisation some such pair finds candidates there
    assert (got["n_candidates"][5:7] > 0).any() and np.array_equal(got["n_candidates"][5:7], exp["n_candidates"][5:7])
    if mode == fn.SIM3 and camera != "kb8":                                            # and more than a wavefront's worth of them
        assert (got["n_candidates"][5:7] > 64).any()
    if camera == "stereo" and mode == fn.CHI2:                                         # both chi2 branches decide something
        mono = fn.shape_case("mono", mode)[2]
        assert (got["n_candidates"] != mono["n_candidates"]).any() and (targets[0].key_uright >= 0).any() and (targets[0].key_uright < 0).any()


@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 300])
@pytest.mark.parametrize("K", [1, 3, 8])
def test_targets_and_points_per_call(matcher, K, P):
    targets, pts, exp = fn.head(*fn.shape_case("stereo", fn.CHI2), K, P)
    got = matcher.fuse_search(targets, pts, fn.CHI2)
    assert got["stage"].shape == (K, P) and fn.same_bits(got, exp) == []


@pytest.mark.parametrize("mode", MODES, ids=["chi2", "sim3"])
def test_constructed_pairs(matcher, mode):
    targets, pts, stages, names, best = fn.constructed_case()
    exp = fn.search(targets, pts, mode)
    got = assert_three_way(matcher, targets, pts, mode, exp, "constructed")
    assert {n: int(s) for n, s in zip(names, got["stage"][0])} == {n: int(s) for n, s in zip(names, stages)}
    at = {n: i for i, n in enumerate(names)}
    for name, idx in best.items():
        assert got["best_idx"][0, at[name]] == idx, name
    assert got["best_dist"][0, at["tie_cells"]] == 3 and got["best_dist"][0, at["tie_one_cell"]] == 4
    assert got["level"][0, at["level_0"]] == 0 and got["n_candidates"][0, at["level_0"]] == 1       # the band [-1, 0] keeps octave 0
    assert got["level"][0, at["level_top"]] == targets[0].n_levels - 1 and got["n_candidates"][0, at["level_top"]] == 2
    assert [int(got["level"][0, at[f"ratio_sf^{k}"]]) for k in (1, 3)] == [1, 3]
    assert not (got["stage"][2] == fn.SEARCHED).any() and (got["stage"][2] == fn.EMPTY).any()   # th = 3e38: the conversion overflows, an early return
    assert got["stage"][1, at["level_0"]] == fn.EMPTY and got["stage"][1, at["level_top"]] == fn.SEARCHED   # off the second target's grid; on it


def test_every_output_word_is_written(matcher):
    """Prefilled with 0xAB bytes / NaN; and an array that is not wanted stays NULL while the others are complete."""
    targets, pts, exp = fn.shape_case("mono", fn.CHI2)
    ct, cp, cr, _keep, out = orb.fuse_args(targets, pts, fill=(np.int32(-1414812757), np.nan))   # 0xABABABAB
    capi.check(matcher.lib.osh_orb_fuse_search(matcher.ctx, len(targets), ct, C.byref(cp), fn.CHI2, C.byref(cr)), "osh_orb_fuse_search", matcher.lib)
    assert fn.same_bits(out, exp) == []
    ct, cp, cr, _keep, out = orb.fuse_args(targets, pts, fill=(np.int32(-1414812757), np.nan))
    cr.u = C.cast(None, capi.c_float_p); cr.n_candidates = C.cast(None, capi.c_int32_p)
    capi.check(matcher.lib.osh_orb_fuse_search(matcher.ctx, len(targets), ct, C.byref(cp), fn.CHI2, C.byref(cr)), "osh_orb_fuse_search", matcher.lib)
    assert sorted(fn.same_bits(out, exp)) == ["n_candidates", "u"] and np.isnan(out["u"]).all()


def test_many_targets_in_one_call_equal_one_call_each(matcher):
    targets, pts, exp = fn.shape_case("kb8", fn.SIM3)
    batch = matcher.fuse_search(targets, pts, fn.SIM3)
    for k, t in enumerate(targets):
        single = matcher.fuse_search([t], pts, fn.SIM3)
        assert all(np.array_equal(single[n][0].view(np.uint8), batch[n][k].view(np.uint8)) for n in fn.NAMES), k
    assert fn.same_bits(batch, exp) == []


def test_an_empty_call(matcher):
    targets, pts, _ = fn.shape_case("mono", fn.CHI2)
    assert matcher.fuse_search([], pts, fn.CHI2)["stage"].shape == (0, 300)
    assert matcher.fuse_search(targets, fn.head(targets, pts, fn.shape_case("mono", fn.CHI2)[2], 8, 0)[1], fn.CHI2)["stage"].shape == (8, 0)


def test_refused_calls_leave_the_context_usable(matcher):
    targets, pts, exp = fn.head(*fn.shape_case("mono", fn.CHI2), 3, 65)

    def refused(match, code, k=0, points=None, mode=fn.CHI2, **change):
        bad = copy.copy(targets)
        bad[k] = dataclasses.replace(targets[k], **change)
        with pytest.raises(capi.OshError, match=match) as e:
            matcher.fuse_search(bad, points or pts, mode)
        assert e.value.code == code
        assert fn.same_bits(matcher.fuse_search(targets, pts, fn.CHI2), exp) == []

    refused("target 2: pose", capi.OSH_ERR_INVALID, k=2, tcw=np.array([0, np.inf, 0], np.float32))
    refused("target 0: th is not finite", capi.OSH_ERR_INVALID, th=float("nan"))
    refused("target 0: keypoint 7: key_octave 8 outside", capi.OSH_ERR_INVALID, key_octave=np.where(np.arange(200) == 7, 8, targets[0].key_octave).astype(np.int32))
    refused("unknown mode 2", capi.OSH_ERR_INVALID, mode=2)
    spot = np.tile(np.array([[100.0, 100.0]], np.float32), (256, 1))
    refused("target 0: 256 keypoints in one grid cell", capi.OSH_ERR_UNSUPPORTED, key_xy=spot, key_octave=np.zeros(256, np.int32), desc=np.zeros((256, 32), np.uint8))


def test_result_does_not_depend_on_what_the_context_ran_before(hip_lib, monkeypatch):
    """The stereo, bag-of-words and FAST entries between calls, in two orders, a larger and a smaller call in turn: the same bits as
    the restatement, which is what a fresh context gives."""
    monkeypatch.setenv("OSH_ZERO_NEW_BUFFERS", "1")
    big = fn.shape_case("stereo", fn.CHI2)
    small = fn.head(*fn.shape_case("kb8", fn.SIM3), 3, 65)
    rect = [ss.make_stereo_frame(301, n_left=65, n_right=257, n_levels=3)]
    fast = [sfa.make_frame(5, n_levels=2)]
    tree = sb.make_vocab(41, k=10, L=4)
    desc = [np.random.default_rng(3).integers(0, 256, (200, 32), dtype=np.uint8)]
    with orb.BowVocab(tree) as vocab:
        others = {"stereo": lambda m: m.stereo_match(rect), "fast": lambda m: m.fast_detect(fast), "bow": lambda m: m.bow_transform(vocab, desc)}
        for order in (("stereo", "fast", "bow"), ("bow", "fast", "stereo")):
            with orb.OrbMatcher(0) as m:
                for k, other in enumerate(order):
                    others[other](m)
                    (targets, pts, exp), mode = (big, fn.CHI2) if k % 2 == 0 else (small, fn.SIM3)
                    assert fn.same_bits(m.fuse_search(targets, pts, mode), exp) == [], (other, order)
                assert fn.same_bits(m.fuse_search(small[0], small[1], fn.SIM3), small[2]) == [], "small after big"


def test_times_are_zero_before_a_call_and_kept_under_profiling(hip_lib):
    targets, pts, _ = fn.shape_case("mono", fn.CHI2)
    with orb.OrbMatcher(0) as m:
        assert np.array_equal(m.fuse_times(), np.zeros(4))
        m.set_profiling(True)
        m.fuse_search(targets, pts, fn.CHI2)
        t = m.fuse_times()
        assert (t >= 0).all() and t.sum() > 0


# ------------------------------------------------------------------------------------------ the class layer, search on the device, the twin through ORBmatcher::Fuse itself
@pytest.mark.parametrize("rig", [False, True], ids=["stereo", "fisheye_rig"])
def test_fuse_batch_equals_the_fuse_calls_one_after_another(hip_lib, rig):
    fc.first_overload(rig, cpu=False)


def test_fuse_batch_sim3_equals_the_fuse_calls_one_after_another(hip_lib):
    fc.sim3_overload(cpu=False)


@pytest.mark.parametrize("with_poses", [True, False], ids=["corrected_poses", "keyframe_list"])
def test_search_and_fuse_equals_the_loop_of_fuse_and_replace(hip_lib, with_poses):
    fc.search_and_fuse(with_poses, cpu=False)


@pytest.mark.parametrize("rig", [False, True], ids=["stereo", "fisheye_rig"])
def test_pack_and_header_agree_with_the_host_part_of_fuse_on_every_pair(hip_lib, rig):
    """Which points are queries, how many candidates each has and the best candidate: FuseBatch's pack searched by osh_orb_fuse_search against
    the projection, gates and candidate lists of ORBmatcher::Fuse itself (the stand-in camera's libm project through an SE3f), for
    every keyframe of the scene, both overloads."""
    n_pairs, n_queries = fc.fuse_pairs_agree(rig, cpu=False)
    assert n_pairs >= 4000 and n_queries >= 1000, (n_pairs, n_queries)
