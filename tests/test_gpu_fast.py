"""osh_orb_fast_detect / osh_orb_ic_angle and ORBextractor::ComputeKeyPointsOctTree on the device against the numpy restatement of
tests/fast_numpy.py: counts, coordinates, responses, cells, moments as integers and the angles as bit patterns, for every corner,
without tolerance."""
import numpy as np
import pytest

import fast_numpy as fn
from orb_slam3_study_kr_amd import capi, host, orb, synth
from orb_slam3_study_kr_amd import synth_fast as sf

pytestmark = pytest.mark.gpu
F = np.float32


def _check(m, names, what, borders=None):
    """One detect call for the named cases, then IC_Angle for their keypoints by token; everything against the restatement."""
    cases = [fn.case(n) for n in names]
    got = m.fast_detect([c[0] for c in cases], borders=borders)
    for k, (frame, exp, _, _) in enumerate(cases):
        assert got[k]["n_out"] == len(exp["level"]) and got[k]["n_cells"] == len(exp["used_min_th"]), f"{what}[{k}] counts"
        fn.assert_detect_same(got[k], exp, f"{what}[{k}]")
    ang = m.ic_angle([dict(xy=c[2][0], level=c[2][1], token=got[k]["token"]) for k, c in enumerate(cases)])
    for k, c in enumerate(cases):
        fn.assert_angles_same(ang[k], c[3], f"{what}[{k}] by token")
    return got, ang


@pytest.mark.parametrize("name", fn.CASE_NAMES)
def test_committed_cases_equal_the_restatement(hip_lib, name):
    frame, _, (kxy, klevel), exp_angle = fn.case(name)
    with orb.OrbMatcher(0) as m:
        for border in (0, 3):
            _check(m, [name], f"{name} border {border}", borders=[border])
            ang = m.ic_angle([dict(xy=kxy, level=klevel, pyramid=frame.pyramid)], borders=[border])
            fn.assert_angles_same(ang[0], exp_angle, f"{name} border {border}, explicit pyramid")


@pytest.mark.parametrize("n_levels", range(1, 9))
def test_one_to_eight_pyramid_levels(hip_lib, n_levels):
    with orb.OrbMatcher(0) as m:
        got, _ = _check(m, [f"levels_{n_levels}"], f"levels={n_levels}")
    assert len(got[0]["level_count"]) == n_levels and got[0]["level_count"][0] > 0


def test_one_752x480_frame_of_eight_levels(hip_lib):
    with orb.OrbMatcher(0) as m:
        got, _ = _check(m, ["vga_752x480_L8"], "752x480", borders=[19])
    assert got[0]["n_cells"] == 700 and got[0]["n_out"] > 5000 and (got[0]["level_count"] > 100).all()


def test_moment_frame(hip_lib):
    frame, xy, level = sf.moment_frame()
    exp = fn.ic_angle(frame.pyramid, xy, level)
    with orb.OrbMatcher(0) as m:
        got = m.ic_angle([dict(xy=xy, level=level, pyramid=frame.pyramid)])[0]
    fn.assert_angles_same(got, exp, "moment frame")
    assert got["angle"][:20].tolist() == [0.0] * 8 + [180.0] * 4 + [90.0] * 4 + [270.0] * 4


MIXED = ["mix_240x180_low_th", "uniform_67", "geom_67x2133", "levels_5", "extreme_th_150x110"]


def test_batches_equal_single_calls(hip_lib):
    with orb.OrbMatcher(0) as m:
        for names, borders in ((["dense_200x150"], None), (["mix_160x120", "levels_3"], [2, 0]), (MIXED, [0, 1, 0, 7, 0])):
            batch, batch_ang = _check(m, names, f"batch of {len(names)}", borders=borders)
            for k, n in enumerate(names):
                one, one_ang = _check(m, [n], f"single {n}")
                fn.assert_detect_same(one[0], batch[k], f"single {n} against the batch")
                fn.assert_angles_same(one_ang[0], batch_ang[k], f"single {n} against the batch")


def test_overflow_returns_counts_and_a_second_call_fills_the_arrays(hip_lib):
    frames = [fn.case(n)[0] for n in ("mix_160x120", "dense_200x150")]
    exps = [fn.case(n)[1] for n in ("mix_160x120", "dense_200x150")]
    n0, n1 = (len(e["level"]) for e in exps)
    c0, c1 = (len(e["used_min_th"]) for e in exps)
    with orb.OrbMatcher(0) as m:
        roomy = m.fast_detect(frames, [(n0 + 100, c0 + 7), (n1 + 1, c1)])
        for k in range(2):
            fn.assert_detect_same(roomy[k], exps[k], f"roomy {k}")
        for caps in ([(0, 0), (0, 0)], [(n0 - 1, c0), (n1, c1)], [(n0, c0), (n1 - 1, c1)], [(n0, c0 - 1), (n1, c1)]):
            cf, cr, _keep, outs = orb.fast_args(frames, caps)
            for o in outs:
                for name in ("xy", "response", "level", "cell", "used_min_th"):
                    o[name][...] = 77
            capi.check(m.lib.osh_orb_fast_detect(m.ctx, 2, cf, cr), "osh_orb_fast_detect", m.lib)
            for k, (cap, cell_cap) in enumerate(caps):
                assert (cr[k].n_out, cr[k].n_cells) == ((n0, c0), (n1, c1))[k] and cr[k].pyramid_token != 0
                assert np.array_equal(outs[k]["level_count"], exps[k]["level_count"])
                if cap < (n0, n1)[k] or cell_cap < (c0, c1)[k]:      # counts without arrays: nothing of the frame is written
                    assert all((outs[k][name] == 77).all() for name in ("xy", "response", "level", "cell", "used_min_th"))
                else:                                                 # the other frame of the same call is complete
                    fn.assert_detect_same(orb._fast_outputs(cr, outs)[k], exps[k], f"caps {caps} frame {k}")
            # the sizes that came back serve the second call
            again = m.fast_detect(frames, [(cr[k].n_out, cr[k].n_cells) for k in range(2)])
            for k in range(2):
                fn.assert_detect_same(again[k], roomy[k], f"second call after {caps}, frame {k}")


def test_tokens(hip_lib):
    a, b, c = (fn.case(n) for n in ("mix_160x120", "dense_200x150", "equal_th_131x97"))
    item = lambda case, **kw: dict(xy=case[2][0], level=case[2][1], **kw)
    with orb.OrbMatcher(0) as m, orb.OrbMatcher(0) as other:
        first = m.fast_detect([a[0], b[0]])
        assert first[1]["token"] == first[0]["token"] + 1
        # a token per frame of the call, in any order, several times, mixed with an explicit pyramid
        got = m.ic_angle([item(b, token=first[1]["token"]), item(c, pyramid=c[0].pyramid), item(a, token=first[0]["token"])])
        for g, case in zip(got, (b, c, a)):
            fn.assert_angles_same(g, case[3], "tokens and a pyramid in one call")
        fn.assert_angles_same(m.ic_angle([item(a, pyramid=a[0].pyramid)])[0], got[2], "explicit pyramid against token")
        fn.assert_angles_same(m.ic_angle([item(b, token=first[1]["token"])])[0], b[3], "the token outlives IC_Angle calls")
        # keypoints are checked against the resident levels: level 1 of `a` is smaller than what fits `b`
        with pytest.raises(capi.OshError) as e:
            m.ic_angle([dict(xy=np.asarray([[150.0, 60.0]], F), level=np.asarray([1], np.int32), token=first[0]["token"])])
        assert e.value.code == capi.OSH_ERR_INVALID and "disc leaves level 1" in str(e.value)
        # another context's token, and a number that was never handed out
        other.fast_detect([c[0]])
        for bad in (first[0]["token"] + 2, 0, 2 ** 63):
            with pytest.raises(capi.OshError) as e:
                m.ic_angle([item(a, token=bad)])
            assert e.value.code == capi.OSH_ERR_INVALID and "token" in str(e.value)
        with pytest.raises(capi.OshError):
            other.ic_angle([item(a, token=first[0]["token"])])
        # a refused detect leaves the resident pyramid; the next accepted one replaces it
        with pytest.raises(capi.OshError):
            m.fast_detect([sf.FastFrame(a[0].pyramid, 7, 8)])
        fn.assert_angles_same(m.ic_angle([item(a, token=first[0]["token"])])[0], a[3], "after a refused detect")
        second = m.fast_detect([c[0]])
        with pytest.raises(capi.OshError) as e:
            m.ic_angle([item(a, token=first[0]["token"])])
        assert "token" in str(e.value)
        fn.assert_angles_same(m.ic_angle([item(c, token=second[0]["token"])])[0], c[3], "the new token")
        fn.assert_detect_same(second[0], c[1], "after the refusals")


@pytest.fixture()
def zero_new_buffers():
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("OSH_ZERO_NEW_BUFFERS", "1")
        yield


def test_long_lived_context_equals_fresh_contexts(hip_lib, zero_new_buffers):
    """A matcher that ran other osh_orb_* calls and larger pyramids first returns, for every later call, bit for bit what a fresh
    matcher returns."""
    later = [["levels_2"], ["uniform_67", "four_corners_67"], MIXED[:3], ["geom_2133x67"], ["mix_160x120"]]
    pair = synth.make_orb_pair(9, 2000, 2000)
    with orb.OrbMatcher(0) as m:
        m.search([pair])
        _check(m, ["vga_752x480_L8", "dense_200x150"], "warm-up")
        for k, names in enumerate(later):
            got, ang = _check(m, names, f"step {k}")
            m.search([pair], windowed=False)
            with orb.OrbMatcher(0) as fresh:
                ref, ref_ang = _check(fresh, names, f"step {k} fresh")
            for j in range(len(names)):
                fn.assert_detect_same(got[j], ref[j], f"step {k} frame {j}")
                fn.assert_angles_same(ang[j], ref_ang[j], f"step {k} frame {j}")


@pytest.mark.parametrize("name,nfeatures,border", [("mix_240x180_low_th", 200, 0), ("mix_240x180_low_th", 5000, 19), ("dense_200x150", 2, 3),
                                                   ("vga_752x480_L8", 1000, 19), ("levels_6", 60, 0)])
def test_compute_keypoints_oct_tree(hip_lib, name, nfeatures, border):
    """ORBextractor::ComputeKeyPointsOctTree of the host layer.  What reaches DistributeOctTree equals the restatement; every
    keypoint that comes back is one of its level's candidates moved by minBorder, with that candidate's response, its level as
    octave, the size of :880 and the restatement's angle.  Which candidates the octree keeps is the test double's business.
    nfeatures = 2 makes the first call's capacity (10 * nfeatures per level) too small: the retry."""
    frame, exp, _, _ = fn.case(name)
    if nfeatures == 2:      # the first call has room for 10 * nfeatures candidates per level: too few, so the retry runs
        assert exp["level_count"].sum() > 10 * nfeatures * frame.n_levels
    r = host.orbextractor_compute_keypoints(frame.pyramid, nfeatures=nfeatures, ini_th=frame.ini_th, min_th=frame.min_th, border=border)
    n_levels = frame.n_levels
    assert np.array_equal(r["cand_level_count"], exp["level_count"])
    assert np.array_equal(r["cand_xy"].view(np.uint32), exp["xy"].view(np.uint32)) and np.array_equal(r["cand_response"], exp["response"])
    assert r["features_per_level"].sum() == nfeatures or nfeatures < n_levels
    sfs = np.cumprod(np.concatenate([[F(1)], np.full(n_levels - 1, F(1.2), F)]), dtype=F)
    assert np.array_equal(r["scale_factors"], sfs)
    first = np.concatenate([[0], np.cumsum(r["level_count"])])
    cand_first = np.concatenate([[0], np.cumsum(exp["level_count"])])
    assert r["level_count"].sum() > 0
    for l in range(n_levels):
        rows, cols = frame.pyramid[l].shape
        if exp["level_count"][l]:
            assert r["cand_args"][l].tolist() == [16, cols - 16, 16, rows - 16, int(r["features_per_level"][l]), l]
        assert r["level_count"][l] <= exp["level_count"][l]
        cand = {(float(x), float(y)): float(v) for (x, y), v in zip(exp["xy"][cand_first[l]:cand_first[l + 1]], exp["response"][cand_first[l]:cand_first[l + 1]])}
        s = slice(first[l], first[l + 1])
        xy = r["xy"][s]
        assert (r["octave"][s] == l).all() and (r["size"][s] == F(int(F(31) * sfs[l]))).all()
        for (x, y), v in zip(xy, r["response"][s]):
            assert cand.get((float(x) - 16.0, float(y) - 16.0)) == float(v), (l, x, y, v)
        assert len({(float(x), float(y)) for x, y in xy}) == len(xy)
        if len(xy):
            ang = fn.ic_angle(frame.pyramid, xy, np.full(len(xy), l, np.int32))["angle"]
            assert np.array_equal(r["angle"][s].view(np.uint32), ang.view(np.uint32)), f"level {l} angles"


def test_a_refused_call_leaves_every_level_empty(hip_lib, capfd):
    """The error path of ORBextractor::ComputeKeyPointsOctTree through calls the C-ABI refuses: thresholds it does not take, and an
    extractor with more levels than its pyramid.  A message on stderr, allKeypoints empty at every level, nothing handed to the
    octree; the next call on the same thread's context is served.

    One branch of the body stays unexecuted by any test: the one that clears allKeypoints when osh_orb_ic_angle fails after the
    octree has run.  The keypoints it sends are candidates of the detector moved by minBorder, whose discs lie inside their levels,
    and the token is the one the detector just returned, so no valid input makes that call refuse; only a device error reaches it,
    and none is provoked here."""
    frame, exp, _, _ = fn.case("mix_160x120")
    for kw, needle in ((dict(ini_th=0, min_th=0), "threshold outside [1, 255]"), (dict(ini_th=5, min_th=9), "min_th 9 > ini_th 5"),
                       (dict(nlevels=4), "the pyramid has 3 of 4 levels")):
        r = host.orbextractor_compute_keypoints(frame.pyramid, **kw)
        assert len(r["level_count"]) == kw.get("nlevels", 3)
        assert (r["level_count"] == 0).all() and (r["cand_level_count"] == 0).all() and len(r["xy"]) == 0
        assert needle in capfd.readouterr().err
    r = host.orbextractor_compute_keypoints(frame.pyramid)
    assert np.array_equal(r["cand_level_count"], exp["level_count"]) and r["level_count"].sum() > 0


def test_time_slots(hip_lib):
    frame, _, (kxy, klevel), _ = fn.case("mix_160x120")
    with orb.OrbMatcher(0) as m:
        assert (m.fast_times() == 0).all() and (m.ic_angle_times() == 0).all()
        m.set_profiling(True)
        got = m.fast_detect([frame])
        m.ic_angle([dict(xy=kxy, level=klevel, token=got[0]["token"])])
        assert (m.fast_times() > 0).all() and (m.ic_angle_times() > 0).all()
