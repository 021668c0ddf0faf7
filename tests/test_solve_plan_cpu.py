"""Which factorisation osh_lba_upload gives the reduced camera systems (csrc/solve_plan.h), on the CPU: ``osh_lba_solve_plan_check``
returns the plan for a window size, a batch size and the three switches; the byte formula of csrc/ldlt_block.h is restated here and
the plan is checked at every boundary, both ways.

The limits are part of what the suite relies on: the tests that mean to run big_solve.h, k_solve<12> or k_solve<6> pick their
window sizes by them.  When ``ldlt_lds_doubles`` changes (it once had two LDS panels, 2 nb W + ..., and NB = 6 stopped fitting at
236 poses) this file fails and says where the limits went."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import capi

BUDGET = 150 * 1024
BATCH_WINDOWS = 128          # from this many windows on a batch takes 256-thread blocks


def plan(poses, n_windows=1, nb=0, threads=0, big=0):
    lib = capi.load_library()
    out = np.full(4, -1, dtype=np.int32)
    rc = lib.osh_lba_solve_plan_check(6 * poses, n_windows, nb, threads, big, capi.ptr(out, capi.c_int32_p))
    assert rc == 0, lib.osh_last_error().decode()
    return dict(big=bool(out[0]), nb=int(out[1]), threads=int(out[2]), lds_bytes=int(out[3]))


# ---- the rule restated
def row_stride(n):
    return (n + 24 + 1) & ~1


def lds_bytes(nb, n, threads):
    """One nb x W panel, x [W], pivots / reciprocals / partials [3 nb], two nb x nb blocks, the cross-wave scratch and the three
    integer lists of the envelope (counted in doubles)."""
    W = row_stride(n)
    return 8 * (nb * W + W + 3 * nb + 2 * nb * nb + threads // 64 + 8 + (W // 32 + 4) + (W // 12 + 2) + (W // (2 * nb) + 2))


def restated(poses, n_windows=1, nb=0, threads=0, big=0):
    n = 6 * poses
    t = 256 if n_windows >= BATCH_WINDOWS else 512
    b = 24
    while b > 6 and lds_bytes(b, n, t) > BUDGET:       # the panel is chosen with the batch's own thread count ...
        b //= 2
    if threads in (256, 512):
        t = threads
    if nb in (24, 12, 6) and nb <= b:
        b = nb
    is_big = bool(big) or lds_bytes(b, n, t) > BUDGET   # ... and has to fit with the thread count that runs
    return dict(big=is_big, nb=6 if is_big else b, threads=t, lds_bytes=0 if is_big else lds_bytes(b, n, t))


def _lds(nb, threads):
    return dict(big=False, nb=nb, threads=threads)


def _sub(p, keys=("big", "nb", "threads")):
    return {k: p[k] for k in keys}


@pytest.mark.parametrize("n_windows,threads", [(1, 512), (127, 512), (128, 256), (512, 256)])
def test_every_boundary_both_ways(n_windows, threads):
    last6 = 438 if threads == 256 else 437               # the cross-wave scratch of 512 threads costs the last pose
    expect = {1: 24, 115: 24, 116: 12, 234: 12, 235: 6, 437: 6}
    for poses, nb in expect.items():
        assert _sub(plan(poses, n_windows)) == _lds(nb, threads), poses
    assert _sub(plan(last6, n_windows)) == _lds(6, threads)
    assert plan(last6 + 1, n_windows)["big"]
    assert plan(439, n_windows)["big"] and plan(440, n_windows)["big"] and plan(4000, n_windows)["big"]
    assert plan(438, n_windows)["big"] == (threads == 512)


def test_plan_equals_the_restated_rule_at_every_size():
    for n_windows in (1, 128):
        for poses in range(0, 460):
            assert plan(poses, n_windows) == restated(poses, n_windows), (poses, n_windows)


def test_lds_bytes_are_the_formula_and_fit_the_budget():
    for poses, nb, t, nw in ((50, 24, 256, 512), (115, 24, 512, 1), (116, 12, 512, 1), (234, 12, 256, 128), (235, 6, 512, 1), (438, 6, 256, 128)):
        p = plan(poses, nw)
        assert p["lds_bytes"] == lds_bytes(nb, 6 * poses, t) <= BUDGET
    # one step wider would not fit: the rule takes the WIDEST panel that does
    assert lds_bytes(24, 6 * 116, 512) > BUDGET and lds_bytes(12, 6 * 235, 512) > BUDGET and lds_bytes(6, 6 * 439, 256) > BUDGET
    assert lds_bytes(24, 6 * 115, 512) <= BUDGET and lds_bytes(12, 6 * 234, 512) <= BUDGET and lds_bytes(6, 6 * 438, 256) <= BUDGET
    assert plan(439)["lds_bytes"] == 0


def test_solve_nb_can_only_narrow():
    for nw in (1, 128):
        assert [plan(40, nw, nb=b)["nb"] for b in (24, 12, 6)] == [24, 12, 6]
        assert [plan(116, nw, nb=b)["nb"] for b in (24, 12, 6)] == [12, 12, 6]      # 24 would not fit: ignored
        assert [plan(235, nw, nb=b)["nb"] for b in (24, 12, 6)] == [6, 6, 6]
        assert not any(plan(p, nw, nb=b)["big"] for p in (40, 116, 235) for b in (24, 12, 6))
        for junk in (-6, 1, 7, 8, 16, 48):
            assert plan(40, nw, nb=junk) == plan(40, nw)
        # a narrower panel never changes whether the system fits at all
        assert plan(439, nw, nb=6)["big"]
    for poses in (1, 40, 116, 235, 437):
        for b in (24, 12, 6):
            assert plan(poses, nb=b) == restated(poses, nb=b)
            assert plan(poses, nb=b)["lds_bytes"] <= plan(poses)["lds_bytes"]


def test_solve_threads_override():
    assert plan(40, 1, threads=256)["threads"] == 256 and plan(40, 512, threads=512)["threads"] == 512
    for junk in (0, 64, 128, 1024, -256):
        assert plan(40, 1, threads=junk) == plan(40, 1) and plan(40, 512, threads=junk) == plan(40, 512)
    # the panel is chosen before the override: the one size at which the two thread counts differ
    assert _sub(plan(438, 128)) == _lds(6, 256)
    assert plan(438, 128, threads=512)["big"] and not plan(438, 1, threads=256)["big"]
    for poses in (40, 116, 235, 437, 438, 439):
        for nw in (1, 128):
            for t in (256, 512):
                assert plan(poses, nw, threads=t) == restated(poses, nw, threads=t)


def test_solve_big_override_selects_the_global_memory_path_at_every_size():
    for poses in (0, 1, 5, 6, 40, 116, 235, 438, 439):
        for nw in (1, 128):
            p = plan(poses, nw, big=1)
            assert p == restated(poses, nw, big=1)
            assert p["big"] and p["lds_bytes"] == 0 and p["nb"] == 6
            assert p["threads"] == plan(poses, nw)["threads"]
    assert plan(40, big=1, nb=12, threads=256) == dict(big=True, nb=6, threads=256, lds_bytes=0)
    assert not plan(40, big=0)["big"]


def test_bad_arguments_are_refused():
    lib = capi.load_library()
    out = np.zeros(4, dtype=np.int32)
    assert lib.osh_lba_solve_plan_check(-6, 1, 0, 0, 0, capi.ptr(out, capi.c_int32_p)) == capi.OSH_ERR_INVALID
    assert lib.osh_lba_solve_plan_check(60, 0, 0, 0, 0, capi.ptr(out, capi.c_int32_p)) == capi.OSH_ERR_INVALID
    assert lib.osh_lba_solve_plan_check(60, 1, 0, 0, 0, None) == capi.OSH_ERR_INVALID
