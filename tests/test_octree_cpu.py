"""ORBextractor::DistributeOctTree without a GPU: the host build of csrc/orb_octree.h (the statements the kernel runs, as arrays and
prefix sums) against the list-based numpy restatement of tests/octree_numpy.py, kept indices and their order bit for bit, on the
lists tests/test_gpu_octree.py runs on the device; a census of what the committed lists hold, computed by the restatement alone; the
refusals of osh_orb_octree_distribute, which need no device; and `make octree-check`."""
import subprocess

import numpy as np
import pytest

import fast_numpy as fn
import octree_numpy as on
from orb_slam3_study_kr_amd import capi, orb

F = np.float32


def _assert_same(got, kept, what):
    assert got["status"] == capi.OSH_OK and got["n_out"] == len(kept), f"{what}: {got['n_out']} kept, {len(kept)} expected"
    assert np.array_equal(got["index"], kept), f"{what}: differs at {np.argwhere(got['index'] != kept)[:5].tolist()}"


@pytest.mark.parametrize("name", on.CASE_NAMES)
def test_host_build_equals_the_restatement(name):
    kept, _ = on.expected(name)
    got, rc, _ = orb.octree_cpu([on.cases()[name]])
    assert rc == capi.OSH_OK
    _assert_same(got[0], kept, name)


@pytest.mark.parametrize("name", fn.CASE_NAMES)
def test_host_build_on_the_candidates_of_the_fast_cases(name):
    lists = on.fast_lists(fn.case(name))
    got, rc, _ = orb.octree_cpu(lists)
    assert rc == capi.OSH_OK
    for l, lst in enumerate(lists):
        _assert_same(got[l], on.distribute(*lst)[0], f"{name} level {l}")


def test_census_of_the_committed_lists():
    """The restatement alone shows, over the committed lists, every path the kernel can get wrong."""
    cs = {name: on.expected(name)[1] for name in on.CASE_NAMES}
    args = {name: on.cases()[name] for name in on.CASE_NAMES}
    n_ini = {c["n_ini"] for c in cs.values() if not c["n_ini_zero"]}
    assert {1, 2, 3} <= n_ini, n_ini
    assert any(c["ratio_half"] for c in cs.values()) and any(c["n_ini_zero"] for c in cs.values())
    assert any(c["finish"] == "A_size" for c in cs.values())
    stalled = [name for name, c in cs.items() if c["finish"] in ("A_prev", "B_prev") and c["multi_left"]]
    assert {"lone_quadrant_128x88", "same_pixel_128x88", "only_same_pixel_128x88"} <= set(stalled), stalled
    assert cs["lone_quadrant_128x88"]["count"] == 1 and cs["lone_quadrant_128x88"]["rounds_a"] == 1
    assert any(c["rounds_b"] >= 1 for c in cs.values()) and any(c["rounds_b"] >= 2 for c in cs.values())
    assert any(c["b_break"] for c in cs.values())
    assert any(c["sort_tied_over_16"] for c in cs.values()) and max(max(c["sort_sizes"], default=0) for c in cs.values()) > 16
    assert sum(c["response_tie"] for c in cs.values()) >= 10
    assert sum(c["beyond_right"] for c in cs.values()) >= 1
    n_features = {a[4] for a in args.values()}
    assert {0, 1} <= n_features and any(a[4] > len(a[1]) for a in args.values())
    assert {0, 1} <= {len(a[1]) for a in args.values()}
    # N + 1 and N + 2 from a round B that breaks (it is entered below N and a division adds at most 3 nodes), N + 3 from the four
    # children of a lone root with N = 1: the three counts above N that max(N + 3, 4 nIni) allows for one root
    over = {c["count"] - args[name][4] for name, c in cs.items() if args[name][4] >= 1}
    assert {1, 2, 3} <= over, over
    assert {1, 2} <= {c["count"] - args[name][4] for name, c in cs.items() if c["finish"] == "B_size"}
    for name, c in cs.items():      # what the header derives: the list length and the rounds
        assert c["count"] <= max(args[name][4] + 3, 4 * c["n_ini"]) and c["rounds_a"] + c["rounds_b"] <= 17, name
    # the kernel's two homes of the keys: LDS up to 2048 candidates, global memory beyond
    assert any(len(a[1]) > 2048 for a in args.values()) and any(1 < len(a[1]) <= 2048 for a in args.values())


def test_overflow_convention_on_the_host():
    lst = on.cases()["grid_130_128x88_n65"]
    kept, _ = on.expected("grid_130_128x88_n65")
    got, rc, _ = orb.octree_cpu([lst, lst], capacities=[len(kept) - 1, len(kept)])
    assert rc == capi.OSH_OK
    assert got[0]["n_out"] == len(kept) and got[0]["index"] is None
    _assert_same(got[1], kept, "exact capacity")


def _refusals():
    xy, r = np.array([[1, 1], [2, 3]], F), np.array([1, 2], F)
    nan, inf = F("nan"), F("inf")

    def bad(i, j, v):
        a = xy.copy()
        a[i, j] = v
        return a

    I, U = capi.OSH_ERR_INVALID, capi.OSH_ERR_UNSUPPORTED
    return [
        ("x nan", (bad(1, 0, nan), r, 10, 10, 5), None, I), ("y inf", (bad(0, 1, inf), r, 10, 10, 5), None, I),
        ("response nan", (xy, np.array([1, nan], F), 10, 10, 5), None, I), ("x == W", (bad(1, 0, F(10)), r, 10, 10, 5), None, I),
        ("x < 0", (bad(0, 0, F(-0.5)), r, 10, 10, 5), None, I), ("y < 0", (bad(0, 1, F(-1)), r, 10, 10, 5), None, I),
        ("W 0", (xy, r, 0, 10, 5), None, I), ("H negative", (xy, r, 10, -4, 5), None, I), ("W above the side limit", (xy, r, capi.OSH_FAST_MAX_SIDE + 1, 10, 5), None, I),
        ("NULL xy", (None, r, 10, 10, 5), 2, I), ("NULL response", (xy, None, 10, 10, 5), 2, I), ("negative n", (xy, r, 10, 10, 5), -1, I),
        ("N above the limit", (xy, r, 10, 10, capi.OSH_OCTREE_MAX_FEATURES + 1), None, U),
        ("nIni above the limit", (xy, r, 650, 10, 5), None, U),
    ]


def test_refusals_need_no_device():
    lib = capi.load_library()
    for what, lst, count, code in _refusals():
        counts = None if count is None else [count]
        cl, cr, _keep, _ = orb.octree_args([lst], counts=counts)
        assert lib.osh_orb_octree_distribute(None, 1, cl, cr) == code, what          # before the missing context is noticed
        assert what and capi.last_error(lib)
        assert orb.octree_cpu([lst], counts=counts)[1] == code, what
    # a valid list at the limits passes the checks and stops at the missing context
    n = capi.OSH_OCTREE_MAX_CANDIDATES
    xy, r = np.zeros((n + 1, 2), F), np.ones(n + 1, F)
    cl, cr, _keep, _ = orb.octree_args([(xy[:n], r[:n], 10, 10, capi.OSH_OCTREE_MAX_FEATURES)])
    assert lib.osh_orb_octree_distribute(None, 1, cl, cr) == capi.OSH_ERR_INVALID and "no context" in capi.last_error(lib)
    cl, cr, _keep, _ = orb.octree_args([(xy, r, 10, 10, 5)])
    assert lib.osh_orb_octree_distribute(None, 1, cl, cr) == capi.OSH_ERR_UNSUPPORTED
    cl, cr, _keep, _ = orb.octree_args([(xy[:2], r[:2], 10, 10, 5)], capacities=[-1])
    assert lib.osh_orb_octree_distribute(None, 1, cl, cr) == capi.OSH_ERR_INVALID
    assert lib.osh_orb_octree_distribute(None, -1, None, None) == capi.OSH_ERR_INVALID
    assert lib.osh_orb_octree_get_times(None, None) == capi.OSH_ERR_INVALID


def test_octree_check_under_the_sanitizers():
    csrc = capi.LIB_PATH.parent
    out = subprocess.run(["make", "-C", str(csrc), "octree-check"], capture_output=True, text=True)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
