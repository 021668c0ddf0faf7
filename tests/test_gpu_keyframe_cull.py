"""osh_orb_keyframe_cull_stage / osh_orb_keyframe_cull_count (the counts of LocalMapping::KeyFrameCulling) on the device against the
restatement of tests/keyframe_cull_numpy.py and against the host build of csrc/keyframe_cull.h, bit for bit: all values are
integers and one float32 comparison."""
import ctypes as C

import numpy as np
import pytest

import keyframe_cull_numpy as kn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_keyframe_cull as sk
from test_keyframe_cull_cpu import same, sequential_by_counts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


def three_way(matcher, pb, removed=(), first=0):
    got = matcher.keyframe_cull_count(removed, first)
    same(got, kn.count_under(pb, removed, first))
    same(got, orb.kfcull_cpu(pb, removed, first)[0])
    return got


def test_thresholds_weights_and_float_decisions(matcher):
    pb = sk.thresholds()
    matcher.keyframe_cull_stage(pb)
    got = three_way(matcher, pb)
    assert (got["n_mps"][0], got["n_redundant"][0]) == (len(sk.REDUNDANT_THRESHOLDS), sum(sk.REDUNDANT_THRESHOLDS))
    pb = sk.weights()
    matcher.keyframe_cull_stage(pb)
    for removed, want in sk.REMOVED_WEIGHTS.items():
        got = three_way(matcher, pb, removed)
        assert (got["n_mps"][0], got["n_redundant"][0]) == (sum(w[0] for w in want), sum(w[1] for w in want))
    for n_mps, n_red, th, want in sk.FLOAT_DECISIONS:
        pb = sk.float_decision(n_mps, n_red, th)
        matcher.keyframe_cull_stage(pb)
        got = three_way(matcher, pb)
        assert (got["n_mps"][0], got["n_redundant"][0], got["redundant"][0]) == (n_mps, n_red, want)


@pytest.mark.parametrize("name", list(sk.SEQUENTIAL))
def test_sequential(matcher, name):
    sc = sk.SEQUENTIAL[name][0]()
    pb = kn.problem_of(sc)
    erasable = [not sc.kfs[k]["not_erase"] for k in sc.covisible]
    matcher.keyframe_cull_stage(pb)
    calls = []

    def count(_pb, removed, first):
        calls.append(first)
        return matcher.keyframe_cull_count(removed, first)
    seen, culled = sequential_by_counts(pb, count, erasable)
    want_seen, want_culled = kn.sequential(pb, erasable)
    assert (seen, culled) == (want_seen, want_culled)
    assert len(calls) == 1 + len(culled)
    assert kn.sequential(pb, erasable if name != "not_erase" else None, snapshot=(name != "not_erase"))[0] != seen


def test_shapes(matcher):
    """Candidates of 1, 63, 64, 65 and 257 slots, runs of 70 and 300 observers, removed indices >= 64, repeats in the set, the same
    set twice, and a smaller set after a larger one: nothing is carried from one count to the next."""
    pb = sk.random_problem(5, [1, 63, 64, 65, 257], n_keyframes=400, seed=3, long_runs=(70, 300))
    matcher.keyframe_cull_stage(pb)
    rng = np.random.default_rng(0)
    big = list(rng.choice(400, 40, replace=False))
    first = three_way(matcher, pb, big)
    again = matcher.keyframe_cull_count(big)
    same(first, again)
    for removed in ([], [64, 399], [7, 7, 7], big[:3], []):
        for start in (0, 3, 5):
            three_way(matcher, pb, removed, start)
    assert len(matcher.keyframe_cull_count([], 5)["n_mps"]) == 0


def test_many_candidates_and_two_slots(matcher):
    pb = sk.random_problem(capi.OSH_KFCULL_MAX_CANDIDATES, 37, n_keyframes=300, seed=5)
    matcher.keyframe_cull_stage(pb)
    three_way(matcher, pb, [0, 5, 127, 200])
    three_way(matcher, pb, [3], 100)
    pb = kn.problem_of(sk.two_slots())
    matcher.keyframe_cull_stage(pb)
    got = three_way(matcher, pb)
    assert (got["n_mps"][0], got["n_redundant"][0], got["redundant"][0]) == (2, 2, 1)


def test_largest_table(matcher):
    """A table of OSH_KFCULL_MAX_KEYFRAMES entries; the last entry and entries above 64 removed."""
    sc = sk.big_table(capi.OSH_KFCULL_MAX_KEYFRAMES)
    pb = kn.problem_of(sc)
    last = capi.OSH_KFCULL_MAX_KEYFRAMES - 1
    assert pb.n_keyframes == last + 1 and last in pb.obs_kf
    matcher.keyframe_cull_stage(pb)
    base = three_way(matcher, pb)
    one = three_way(matcher, pb, [last])
    assert base["n_redundant"][0] + base["n_redundant"][1] > one["n_redundant"][0] + one["n_redundant"][1]
    three_way(matcher, pb, [last, 64, 65, 1000, 4000])
    same(three_way(matcher, pb), base)


def test_refusals_with_a_context(matcher):
    lib = matcher.lib
    pb = sk.thresholds()
    matcher.keyframe_cull_stage(pb)
    out, cr = orb.kfcull_result(4)
    rm = np.array([pb.n_keyframes], np.int32)   # inside the mask, outside the staged table
    assert lib.osh_orb_keyframe_cull_count(matcher.ctx, 1, capi.ptr(rm, capi.c_int32_p), 0, C.byref(cr)) == capi.OSH_ERR_INVALID
    assert lib.osh_orb_keyframe_cull_count(matcher.ctx, 0, None, pb.n_candidates + 1, C.byref(cr)) == capi.OSH_ERR_INVALID
    bad = sk.thresholds()
    bad.obs_weight = bad.obs_weight.copy()
    bad.obs_weight[0] = 0
    with pytest.raises(capi.OshError):
        matcher.keyframe_cull_stage(bad)
    three_way(matcher, pb)   # the refused stage left the staged problem and the context usable
    with orb.OrbMatcher(0) as fresh:   # a count before any stage
        assert lib.osh_orb_keyframe_cull_count(fresh.ctx, 0, None, 0, C.byref(cr)) == capi.OSH_ERR_INVALID


def test_times(matcher):
    pb = sk.random_problem(4, 50, seed=1)
    matcher.set_profiling(True)
    try:
        matcher.keyframe_cull_stage(pb)
        matcher.keyframe_cull_count([1])
        ms = matcher.keyframe_cull_times()
    finally:
        matcher.set_profiling(False)
    assert (ms > 0).all()
