"""osh_orb_octree_distribute and ORBextractor::DistributeOctTreeDevice on the device against the list-based numpy restatement of
tests/octree_numpy.py: the kept input indices and their order, bit for bit, on the lists tests/test_octree_cpu.py runs on the host."""
import numpy as np
import pytest

import fast_numpy as fn
import octree_numpy as on
from orb_slam3_study_kr_amd import capi, host, orb

pytestmark = pytest.mark.gpu
F = np.float32


def _assert_same(got, kept, what):
    assert got["status"] == capi.OSH_OK and got["n_out"] == len(kept), f"{what}: {got['n_out']} kept, {len(kept)} expected"
    assert np.array_equal(got["index"], kept), f"{what}: differs at {np.argwhere(got['index'] != kept)[:5].tolist()}"


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


@pytest.mark.parametrize("name", on.CASE_NAMES)
def test_committed_lists_equal_the_restatement(matcher, name):
    _assert_same(matcher.octree_distribute([on.cases()[name]])[0], on.expected(name)[0], name)


@pytest.mark.parametrize("name", fn.CASE_NAMES)
def test_candidates_of_the_fast_cases(matcher, name):
    lists = on.fast_lists(fn.case(name))      # every level of the frame in one call, N from mnFeaturesPerLevel
    got = matcher.octree_distribute(lists)
    assert len(got) == len(lists)
    for l, lst in enumerate(lists):
        _assert_same(got[l], on.distribute(*lst)[0], f"{name} level {l}")


MIXED = ("level_720x448", "empty_128x88", "clusters_128x88_tight", "single_128x88", "portrait_40x100", "wide_300x100", "same_pixel_128x88",
         "n0_features_128x88", "level_720x448", "one_row_60x1")


def test_a_batch_of_mixed_lists_equals_the_single_calls(matcher):
    batch = matcher.octree_distribute([on.cases()[n] for n in MIXED])
    for k, name in enumerate(MIXED):
        _assert_same(batch[k], on.expected(name)[0], f"batch[{k}] {name}")
        one = matcher.octree_distribute([on.cases()[name]])[0]
        assert one["n_out"] == batch[k]["n_out"] and np.array_equal(one["index"], batch[k]["index"]), name


def test_overflow_convention(matcher):
    name = "grid_130_128x88_n65"
    kept = on.expected(name)[0]
    lst = on.cases()[name]
    got = matcher.octree_distribute([lst, lst, lst], capacities=[len(kept) - 1, len(kept), 0])
    assert got[0]["n_out"] == len(kept) and got[0]["index"] is None and got[2]["n_out"] == len(kept) and got[2]["index"] is None
    _assert_same(got[1], kept, "exact capacity")


def test_limits_are_refused_and_the_context_stays_usable(matcher):
    xy, r = np.array([[1, 1], [2, 3]], F), np.array([1, 2], F)
    n = capi.OSH_OCTREE_MAX_CANDIDATES + 1
    for what, lst, code in (("N above the limit", (xy, r, 10, 10, capi.OSH_OCTREE_MAX_FEATURES + 1), capi.OSH_ERR_UNSUPPORTED),
                            ("candidates above the limit", (np.zeros((n, 2), F), np.ones(n, F), 10, 10, 5), capi.OSH_ERR_UNSUPPORTED),
                            ("nIni above the limit", (xy, r, 650, 10, 5), capi.OSH_ERR_UNSUPPORTED),
                            ("x outside the area", (xy + F(9), r, 10, 10, 5), capi.OSH_ERR_INVALID)):
        with pytest.raises(capi.OshError) as e:
            matcher.octree_distribute([on.cases()["single_128x88"], lst])
        assert e.value.code == code, what
    name = "wide_200x100"
    _assert_same(matcher.octree_distribute([on.cases()[name]])[0], on.expected(name)[0], "after the refusals")


def test_n_features_at_the_limit(matcher):
    """N = OSH_OCTREE_MAX_FEATURES on more candidates than that: the longest list the kernel holds."""
    rng = np.random.default_rng(77)
    lst = on._grid_points(rng, 2600, 720, 448, max_response=200) + (720, 448, capi.OSH_OCTREE_MAX_FEATURES)
    kept = on.distribute(*lst)[0]
    assert len(kept) > 1500
    _assert_same(matcher.octree_distribute([lst])[0], kept, "N = 2048")


def test_phase_times(matcher):
    matcher.set_profiling(True)
    try:
        matcher.octree_distribute([on.cases()["grid_500_128x88"]])
        ms = matcher.octree_times()
    finally:
        matcher.set_profiling(False)
    assert ms.shape == (4,) and (ms >= 0).all() and ms[2] > 0


@pytest.mark.parametrize("name", ("grid_500_128x88", "half_ratio_150x100", "lone_quadrant_128x88", "empty_128x88", "level_720x448"))
def test_distribute_octtree_device_through_the_class(hip_lib, name):
    xy, r, W, H, N = on.cases()[name]
    kept = on.expected(name)[0]
    got = host.orbextractor_distribute_device(xy, r, W, H, N)
    assert got["distribute_calls"] == 0                       # the member never goes through DistributeOctTree
    assert np.array_equal(got["index"], kept), name
    assert np.array_equal(got["xy"].view(np.uint32), xy[kept].view(np.uint32)) and np.array_equal(got["response"], r[kept])


def test_distribute_octtree_device_beyond_the_limits_runs_on_the_host(hip_lib, capfd):
    rng = np.random.default_rng(5)
    xy, r = on._grid_points(rng, 300, 700, 10)                 # nIni = 70: more roots than the kernel takes
    kept = on.distribute(xy, r, 700, 10, 120)[0]
    got = host.orbextractor_distribute_device(xy, r, 700, 10, 120)
    assert np.array_equal(got["index"], kept) and got["distribute_calls"] == 0
    assert "on the host" in capfd.readouterr().err
