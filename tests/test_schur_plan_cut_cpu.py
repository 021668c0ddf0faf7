"""Schur work plan (csrc/schur_plan.h) cut at up to 256 landmarks per item, what a call of more than 128 windows uses: the size classes
of ``item_max_lm`` at each boundary, the covering property of tests/test_schur_plan_cpu.py (every observer pair exactly once, the
contribution slots of a block contiguous: ``osh_lba_schur_plan_stats_cut`` refuses a plan that breaks either) at caps 65, 128 and 256,
and where the cut falls: in a group of exactly 256, 257 and 2 x 256 + 1 landmarks with one observer set, and in the middle of a
group that was merged into a running item.  CPU only; the cut is an argument, not an environment variable."""
import numpy as np
import pytest

from orb_slam3_study_kr_amd import capi, lba, synth


def structure_window(n_free, n_fixed, groups):
    """A window with ``count`` landmarks per (observer set, count) of ``groups``, landmarks in that order.  Only its structure
    matters here (the plan does not look at the numbers)."""
    ep, el = [], []
    lm = 0
    for poses, count in groups:
        for _ in range(count):
            for p in sorted(poses):
                ep.append(p); el.append(lm)
            lm += 1
    E, K = len(ep), n_free + n_fixed
    qt = np.zeros((K, 7)); qt[:, 3] = 1.0
    return synth.LbaWindow(n_free=n_free, n_fixed=n_fixed, pose_qt=qt, pose_cam=np.tile([500.0, 500.0, 320.0, 240.0, 40.0], (K, 1)),
                           points=np.tile([0.0, 0.0, 5.0], (lm, 1)), edge_pose=np.array(ep, dtype=np.int32), edge_point=np.array(el, dtype=np.int32),
                           edge_kind=np.full(E, capi.OSH_EDGE_STEREO, dtype=np.uint8), edge_obs=np.tile([320.0, 240.0, 312.0], (E, 1)),
                           edge_info=np.ones(E)).normalise()


def observer_counts(w):
    return np.bincount(w.edge_point[w.edge_pose < w.n_free], minlength=w.n_points)


def check_plan(w, cap):
    """the assertions of tests/test_schur_plan_cpu.py on the plan cut at ``cap``; returns {(sym, nx, ny, landmarks): items}"""
    st = lba.schur_plan_check(w, cap)      # raises unless every observer pair is covered once and every slot lies in its block's range
    k = observer_counts(w)
    assert st["useful_blocks"] == int((k * (k + 1) // 2).sum())
    assert st["reduce_entries"] == w.n_free * (w.n_free + 1) // 2 + w.n_free
    parts = np.maximum(1, (k + 7) // 8)
    assert st["records"] == int((parts * (parts + 1) // 2).sum())
    assert (st["items"] > st["sym_items"]) == bool((k > 8).any())
    shapes = lba.schur_plan_shapes(w, cap)[0]
    assert sum(shapes.values()) == st["items"] and sum(lm * c for (_, _, _, lm), c in shapes.items()) == st["records"]
    assert max(lm for (_, _, _, lm) in shapes) <= cap
    return shapes


@pytest.mark.parametrize("nw, item, chunk", [(1, 24, 256), (2, 24, 256), (3, 32, 512), (8, 32, 512), (9, 64, 1024), (127, 64, 1024), (128, 64, 1024),
                                              (129, 256, 1024), (256, 256, 1024), (512, 256, 1024)])
def test_size_classes_at_each_boundary(nw, item, chunk, monkeypatch):
    monkeypatch.delenv("OSH_LBA_ITEM_MAX", raising=False)
    monkeypatch.delenv("OSH_LBA_CHUNK_EDGES", raising=False)
    assert lba.pack_cuts(nw) == (item, chunk) and lba.pack_cuts(nw, use_env=True) == (item, chunk)
    monkeypatch.setenv("OSH_LBA_ITEM_MAX", "256")
    assert lba.pack_cuts(nw) == (item, chunk) and lba.pack_cuts(nw, use_env=True) == (256, chunk)
    for bad in ("7", "257", "x"):          # outside 8 .. 256: not applied
        monkeypatch.setenv("OSH_LBA_ITEM_MAX", bad)
        assert lba.pack_cuts(nw, use_env=True) == (item, chunk)


def test_the_argument_not_the_environment_cuts_the_checked_plan(monkeypatch):
    w = structure_window(3, 1, [({0, 1, 2, 3}, 300)])
    monkeypatch.setenv("OSH_LBA_ITEM_MAX", "16")
    assert set(check_plan(w, 256)) == {(1, 3, 3, 256), (1, 3, 3, 44)}
    assert lba.pack_check([w, w], item_max=256)["items"] == 4 and lba.pack_check([w, w], item_max=128)["items"] == 6
    assert lba.pack_check([w, w])["items"] == 2 * 19                # no argument: the environment, as an upload
    for bad in (7, 257):
        with pytest.raises(RuntimeError, match="item_max"):
            lba.schur_plan_check(w, bad)
        with pytest.raises(RuntimeError, match="item_max"):
            lba.pack_check([w], item_max=bad)
    with pytest.raises(RuntimeError, match="item_max"):
        lba.schur_plan_shapes(w, 257)


@pytest.mark.parametrize("group, items", [(256, [256]), (257, [256, 1]), (513, [256, 256, 1])])
def test_a_group_of_exactly_the_cap_one_more_and_twice_and_one(group, items):
    # observer set {0, 1, 2}: three row poses, two tiles; the set {0, 1} that follows has one tile and starts an item of its own
    w = structure_window(3, 1, [({0, 1, 3}, 40), ({0, 1, 2, 3}, group)])
    shapes = check_plan(w, 256)
    assert shapes == {**{(1, 3, 3, n): items.count(n) for n in set(items)}, (1, 2, 2, 40): 1}
    for cap in (65, 128):
        got = check_plan(w, cap)
        assert sum(c for (s, nx, ny, lm), c in got.items() if nx == 3) == -(-group // cap)


def test_a_merged_item_reaches_the_cap_in_the_middle_of_a_group():
    # {0, 1, 2} and {0, 1, 3} unite to four poses on the same two tiles: one running item of 200 + 150 landmarks, cut at 256, in the
    # second group; both parts carry the united pose set
    w = structure_window(4, 1, [({0, 1, 2, 4}, 200), ({0, 1, 3, 4}, 150)])
    assert check_plan(w, 256) == {(1, 4, 4, 256): 1, (1, 4, 4, 94): 1}
    # at a cap the first group alone reaches, the second does not join it (a group joins a running item only below the cap)
    assert check_plan(w, 128) == {(1, 3, 3, 128): 2, (1, 3, 3, 72): 1, (1, 3, 3, 22): 1}
    assert check_plan(w, 65) == {(1, 3, 3, 65): 5, (1, 3, 3, 5): 1, (1, 3, 3, 20): 1}
    # a third group joins the item that is already past the cap no more: it starts its own
    w = structure_window(4, 1, [({0, 1, 2, 4}, 200), ({0, 1, 3, 4}, 150), ({0, 2, 3, 4}, 30)])
    assert check_plan(w, 256) == {(1, 4, 4, 256): 1, (1, 4, 4, 94): 1, (1, 3, 3, 30): 1}


@pytest.mark.parametrize("maker", [
    lambda: synth.make_config2(100),
    lambda: synth.make_window(9301, n_free=3, n_fixed=1, n_points=500, stereo=True, track_len=(3, 4)),
    lambda: synth.make_window(9304, n_free=12, n_fixed=1, n_points=500, stereo=True, track_len=(9, 12)),      # 9-12 observers: cross items
    lambda: synth.make_window(6, n_free=40, n_fixed=4, n_points=2000, track_len=(10, 30), obs_dropout=0.3),   # > 16 observers
])
@pytest.mark.parametrize("cap", [65, 128, 256])
def test_plan_covers_every_observer_pair_once(maker, cap):
    w = maker()
    check_plan(w, cap)
    lba.pack_check([w], item_max=cap, chunk_edges=1024)


def test_the_headline_window_at_the_cut_of_a_large_batch():
    """What the rule is for (schur_plan.h): a config-2 window has less than half the symmetric items and 0.57 of the contributions
    at 256 that it has at 64."""
    w = synth.make_config2(100)
    at64, at256 = lba.schur_plan_check(w, 64), lba.schur_plan_check(w, 256)
    assert (at64["sym_items"], at64["items"] - at64["sym_items"], at64["contributions"], at64["rhs_contributions"]) == (301, 85, 7836, 1596)
    assert (at256["sym_items"], at256["items"] - at256["sym_items"], at256["contributions"], at256["rhs_contributions"]) == (141, 82, 4467, 707)
    assert max(lm for (_, _, _, lm) in lba.schur_plan_shapes(w, 256)[0]) == 256
