"""osh_orb_refresh_map_points (MapPoint::ComputeDistinctiveDescriptors and UpdateNormalAndDepth for batches of map points) on the
device against the numpy restatement (tests/mappoint_numpy.py) and the header's host build, bit for bit on every output; and
MapPoint::RefreshBatch, LocalMapping::SearchInNeighbors and LocalMapping::ProcessNewKeyFrame through their signatures on small
stand-in maps."""
import dataclasses

import numpy as np
import pytest

import mappoint_numpy as mn
from orb_slam3_study_kr_amd import capi, host, orb, synth
from orb_slam3_study_kr_amd import synth_bow as sb
from orb_slam3_study_kr_amd import synth_fast as sfa
from orb_slam3_study_kr_amd import synth_mappoints as sm
from orb_slam3_study_kr_amd import synth_stereo as ss

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def matcher(hip_lib):
    with orb.OrbMatcher(0) as m:
        yield m


def head(b, n):
    """The first n points of a batch."""
    e = int(b.entry_off[n])
    return dataclasses.replace(b, entry_off=b.entry_off[:n + 1], desc=b.desc[:e], centre=b.centre[:e], use_desc=b.use_desc[:e], pos=b.pos[:n],
                               ref_centre=b.ref_centre[:n], level_scale=b.level_scale[:n], top_scale=b.top_scale[:n])


def cut(e, n):
    return {k: v[:n] for k, v in e.items()}


def assert_three_way(matcher, b, e, what):
    got = matcher.refresh_map_points([b])[0]
    assert mn.same_bits(got, e) == [], what
    assert mn.same_bits(got, orb.mappoint_cpu([b])[0][0]) == [], what
    return got


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_generator_cases_equal_the_restatement_and_the_host_build(matcher, seed):
    b, e = mn.generator_case(seed)
    assert_three_way(matcher, b, e, f"seed {seed}")


def test_listed_entry_counts(matcher):
    """M in {1, 2, 3, 4, 5, 63, 64, 65, 128, limit}, two points each, points without entries between them."""
    b, e = mn.shapes_case()
    assert sorted(set(b.counts())) == [0] + list(mn.COUNTS) and mn.LIMIT == capi.OSH_MAPPOINT_MAX_DESCRIPTORS
    got = assert_three_way(matcher, b, e, "shapes")
    assert (got["best_entry"][b.counts() > 0] >= 0).any()


def test_special_points(matcher):
    b, e, at = mn.special_case()
    got = assert_three_way(matcher, b, e, "special")
    for name in ("unused", "unused65"):
        assert got["best_entry"][at[name]] == -1 and np.abs(got["normal"][at[name]]).sum() > 0
    p = at["empty"]
    assert got["best_entry"][p] == -1 and not got["normal"][p].any() and got["min_distance"][p] == 0 and got["max_distance"][p] == 0
    assert got["best_entry"][at["identical"]] == 0 and got["best_entry"][at["identical65"]] == 0
    assert got["best_entry"][at["tie"]] == 1 and got["best_median"][at["tie"]] == 40


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_points_per_batch(matcher, n):
    b, e = mn.generator_case(4, 1000)
    got = matcher.refresh_map_points([head(b, n)])[0]
    assert got["best_entry"].shape == (n,) and got["normal"].shape == (n, 3)
    assert mn.same_bits(got, cut(e, n)) == []


def test_three_batches_with_an_empty_one_in_the_middle_equal_the_single_calls(matcher):
    a, c = mn.generator_case(1)[0], mn.shapes_case()[0]
    batch = matcher.refresh_map_points([a, sm.empty_batch(), c])
    assert [o["best_entry"].shape[0] for o in batch] == [a.n_points, 0, c.n_points]
    assert mn.same_bits(batch[0], matcher.refresh_map_points([a])[0]) == [] and mn.same_bits(batch[0], mn.generator_case(1)[1]) == []
    assert mn.same_bits(batch[2], matcher.refresh_map_points([c])[0]) == [] and mn.same_bits(batch[2], mn.shapes_case()[1]) == []


def test_an_empty_call(matcher):
    assert matcher.refresh_map_points([]) == []
    empty = matcher.refresh_map_points([sm.empty_batch(), sm.empty_batch()])
    assert [o["best_entry"].shape for o in empty] == [(0,), (0,)]


def test_every_wanted_output_word_is_written(matcher):
    """Prefilled with 0xAB bytes / NaN: every word of every wanted array is written, points without entries included; an array
    that is not wanted stays NULL and the others are still complete."""
    b, e = mn.shapes_case()
    cb, cr, _keep, outs = orb.mappoint_args([b], fill=(np.int32(-1414812757), np.nan))   # 0xABABABAB
    capi.check(matcher.lib.osh_orb_refresh_map_points(matcher.ctx, 1, cb, cr), "osh_orb_refresh_map_points", matcher.lib)
    assert mn.same_bits(outs[0], e) == []
    for want in (("normal",), ("best_entry", "max_distance")):
        cb, cr, _keep, outs = orb.mappoint_args([b], want=want, fill=(np.int32(-1414812757), np.nan))
        capi.check(matcher.lib.osh_orb_refresh_map_points(matcher.ctx, 1, cb, cr), "osh_orb_refresh_map_points", matcher.lib)
        assert sorted(outs[0]) == sorted(want) and mn.same_bits(outs[0], e, want) == []


def test_refused_calls_leave_the_context_usable(matcher):
    b, e = mn.generator_case(2)
    over = sm.make_batch(5, counts=[3, mn.LIMIT + 1])
    with pytest.raises(capi.OshError, match=f"batch 1: point 1 has {mn.LIMIT + 1} entries"):
        matcher.refresh_map_points([b, over])
    assert mn.same_bits(matcher.refresh_map_points([b])[0], e) == []
    small = sm.make_batch(5, counts=[3, 4])
    centre = small.centre.copy()
    centre[4] = small.centres.shape[0] + 7
    with pytest.raises(capi.OshError, match="batch 0: point 1: entry 1: centre index"):
        matcher.refresh_map_points([dataclasses.replace(small, centre=centre)])
    assert mn.same_bits(matcher.refresh_map_points([b])[0], e) == []
    with pytest.raises(capi.OshError, match="batch 0: point 0: ref_centre -1"):
        matcher.refresh_map_points([dataclasses.replace(small, ref_centre=np.array([-1, 0], np.int32))])
    assert mn.same_bits(matcher.refresh_map_points([b])[0], e) == []


def test_result_does_not_depend_on_what_the_context_ran_before(hip_lib, monkeypatch):
    """The stereo, bag-of-words and FAST entries between calls, in two orders, larger and smaller batches first: the same bits as
    on a fresh context."""
    monkeypatch.setenv("OSH_ZERO_NEW_BUFFERS", "1")
    big, small = [mn.generator_case(1)[0], mn.shapes_case()[0]], [head(mn.generator_case(2)[0], 65)]
    ref_big, ref_small = [mn.generator_case(1)[1], mn.shapes_case()[1]], [cut(mn.generator_case(2)[1], 65)]
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
                    batches, ref = (big, ref_big) if k % 2 == 0 else (small, ref_small)
                    for got, r in zip(m.refresh_map_points(batches), ref):
                        assert mn.same_bits(got, r) == [], (other, order)
                for got, r in zip(m.refresh_map_points(small), ref_small):
                    assert mn.same_bits(got, r) == [], "small after big"
                with orb.OrbMatcher(0) as fresh:        # the other entries are not disturbed either
                    a, b = m.stereo_match(rect)[0], fresh.stereo_match(rect)[0]
                assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def test_times_are_zero_before_a_call_and_kept_under_profiling(hip_lib):
    b, _ = mn.generator_case(1)
    with orb.OrbMatcher(0) as m:
        assert np.array_equal(m.refresh_map_points_times(), np.zeros(4))
        m.set_profiling(True)
        m.refresh_map_points([b])
        t = m.refresh_map_points_times()
        assert (t >= 0).all() and t.sum() > 0


# ------------------------------------------------------------------------------------------ through the signatures
KEYS = ("normal", "min_distance", "max_distance")


def snapshot(g, n_kf):
    return dict(matches=[g.kf_matches(k).tolist() for k in range(n_kf)], obs=[g.mp_observations(j) for j in range(g.n_mp)],
                state=[{k: v for k, v in g.mp_state(j).items() if k != "fuse_candidate_for"} for j in range(g.n_mp)])


def consistent_octaves(w):
    """The window's keypoint levels (random in the generator) replaced by levels that follow the distance, as an image pyramid
    gives them: level = round(log(12.5 m / distance) / log(1.2)).  The level MapPoint::PredictScale expects in another keyframe is
    then the keypoint's own or the one above, which is the band ORBmatcher::Fuse accepts."""
    centre = np.array([-synth.quat_to_R(q[:4]).T @ q[4:] for q in np.asarray(w.pose_qt, np.float64)])
    d = np.linalg.norm(np.asarray(w.points, np.float64)[w.edge_point] - centre[w.edge_pose], axis=1)
    level = np.clip(np.round(np.log(12.5 / d) / np.log(1.2)), 0, synth.N_LEVELS - 1).astype(np.int64)
    w.edge_info = synth.INV_LEVEL_SIGMA2[level].astype(np.float64)


def make_scene(rig: bool, seed: int = 17):
    """Seven keyframes of about 150 features.  Every point is refreshed once so that the gates of Fuse have something to read; then
    observations are taken out (a fusion adds them again) and duplicates are made (a fusion replaces one by the other), and the
    touched points refreshed again.  bad keyframe 6 stays an observer."""
    kw = dict(n_free=5, n_fixed=2, n_points=160, pixel_noise=False, outlier_frac=0.0, point_noise=0.0, pose_noise=(0.0, 0.0))
    w = synth.make_rig_window(seed, **kw) if rig else synth.make_window(seed, stereo=True, **kw)
    consistent_octaves(w)
    g = host.HostGraph(w)
    g.set_mapping(seed=seed)
    g.n_mp = w.n_points
    g.refresh_batch(np.arange(w.n_points))
    rng = np.random.default_rng(seed)
    seen = [[kf for kf, _, _ in g.mp_observations(j)] for j in range(w.n_points)]
    touched = []
    for j in range(w.n_points):
        if len(seen[j]) < 5:
            continue
        r = rng.random()
        if r < 0.3:                                   # forget it in one or two keyframes
            for kf in rng.choice(seen[j], size=int(rng.integers(1, 3)), replace=False):
                g.unlink(int(kf), j)
            touched.append(j)
        elif r < 0.5:                                 # a duplicate that holds it in two of its keyframes
            touched += [j, g.clone_point(j, 5000 + j, rng.choice(seen[j], size=2, replace=False))]
            g.n_mp += 1
    g.refresh_batch(touched)
    g.set_bad(kf=6)
    # covisibility: the current keyframe (4) sees 0..3 (set by HostGraph); second neighbours add 5, skip the current one, a
    # keyframe already listed and the bad one
    g.set_covisible(0, [5, 4, 1, 6])
    g.set_covisible(1, [6, 5, 0])
    g.model_cov = {4: [0, 1, 2, 3], 0: [5, 4, 1, 6], 1: [6, 5, 0], 2: [], 3: [], 5: [], 6: []}
    return g


def model_targets(g, cur, bad, abort=False):
    """vpTargetKFs of src/LocalMapping.cc:746-776 (not inertial)."""
    targets, marked = [], set()
    for k in g.model_cov[cur][:10]:
        if k in bad or k in marked:
            continue
        targets.append(k); marked.add(k)
    for i in range(len(targets)):
        for k2 in g.model_cov[targets[i]][:20]:
            if k2 in bad or k2 in marked or k2 == cur:
                continue
            targets.append(k2); marked.add(k2)
        if abort:
            break
    return targets


def fuse_in_sequence(g, cur, targets, rig, first_loop_only=False):
    """The Fuse calls of SearchInNeighbors (:796-833), one after another through the wrapper of a single call."""
    matches = g.kf_matches(cur).copy()
    for t in targets:
        g.fuse(t, matches, 3.0, False)
        if rig:
            g.fuse(t, matches, 1.0, False)            # Fuse(pKFi, vpMapPointMatches, true): th = 1, the left camera again
    if first_loop_only:
        return []
    cands, marked = [], set()
    for t in targets:
        for j in g.kf_matches(t):
            if j < 0 or g.mp_state(int(j))["bad"] or int(j) in marked:
                continue
            marked.add(int(j)); cands.append(int(j))
    g.fuse(cur, cands, 3.0, False)
    if rig:
        g.fuse(cur, cands, 1.0, False)
    return cands


@pytest.mark.parametrize("rig", [False, True], ids=["stereo", "fisheye_rig"])
def test_search_in_neighbors_through_the_class(hip_lib, rig):
    g, twin = make_scene(rig), make_scene(rig)
    try:
        cur, bad = g.cur, {6}
        assert snapshot(g, 7) == snapshot(twin, 7)
        before = [g.mp_refresh(j) for j in range(g.n_mp)]
        obs_before = [g.mp_observations(j) for j in range(g.n_mp)]
        g.search_in_neighbors(cur)
        targets = model_targets(g, cur, bad)
        assert targets == [0, 1, 2, 3, 5]
        cur_id = int(g.kf_id[cur])
        for k in range(7):                                        # the marks are the reference's
            assert (g.kf_state(k)["fuse_target_for"] == cur_id) == (k in targets), k
        cands = fuse_in_sequence(twin, cur, targets, rig)
        after, expect = snapshot(g, 7), snapshot(twin, 7)
        assert after == expect                                     # the map the same Fuse calls in sequence leave
        gained = sum(len(a) - len(b) for a, b in zip(after["obs"], obs_before) if len(a) > len(b))
        replaced = sum(s["replaced"] >= 0 for s in after["state"])
        assert gained >= 10 and replaced >= 5, (gained, replaced)  # the fusion did both of its jobs
        assert len(cands) >= 100
        for j in range(g.n_mp):                                    # the candidate marks are the reference's
            assert (g.mp_state(j)["fuse_candidate_for"] == cur_id) == (j in cands), j
        refreshed = [int(j) for j in g.kf_matches(cur) if j >= 0 and not g.mp_state(int(j))["bad"]]
        assert len(refreshed) >= 100
        for j in range(g.n_mp):
            now, twin_now = g.mp_refresh(j), twin.mp_refresh(j)
            n = refreshed.count(j)
            # each occurrence counted once (the twin counts what Fuse and MapPoint::Replace call on their own)
            assert now["desc_updates"] - twin_now["desc_updates"] == n and now["normal_updates"] - twin_now["normal_updates"] == n, j
            if n:
                mn.assert_point_is_refreshed(g, j, bad)
            else:                                                  # other points are untouched
                assert np.array_equal(now["desc"], before[j]["desc"]) and all(now[k].tobytes() == before[j][k].tobytes() for k in KEYS), j
        changed = sum(any(g.mp_refresh(j)[k].tobytes() != before[j][k].tobytes() for k in KEYS) for j in set(refreshed))
        assert changed >= 10                                       # and the refresh had something to do
        assert g.kf_state(cur)["connection_updates"] == 1 and all(g.kf_state(k)["connection_updates"] == 0 for k in range(7) if k != cur)
    finally:
        g.close(); twin.close()


@pytest.mark.parametrize("rig", [False, True], ids=["stereo", "fisheye_rig"])
def test_search_in_neighbors_returns_after_the_first_fuse_loop_on_abort(hip_lib, rig):
    g, twin = make_scene(rig), make_scene(rig)
    try:
        cur = g.cur
        before = [g.mp_refresh(j) for j in range(g.n_mp)]
        g.search_in_neighbors(cur, abort_ba=True)
        targets = model_targets(g, cur, {6}, abort=True)
        assert targets == [0, 1, 2, 3, 5]                          # the second neighbours of the first target only: 1's add nothing new here
        fuse_in_sequence(twin, cur, targets, rig, first_loop_only=True)
        assert snapshot(g, 7) == snapshot(twin, 7)
        for j in range(g.n_mp):                                    # nothing refreshed, no candidate marked, no UpdateConnections
            now, twin_now = g.mp_refresh(j), twin.mp_refresh(j)
            assert now["desc_updates"] == twin_now["desc_updates"] and now["normal_updates"] == twin_now["normal_updates"], j
            assert np.array_equal(now["desc"], before[j]["desc"]) and all(now[k].tobytes() == before[j][k].tobytes() for k in KEYS), j
            assert g.mp_state(j)["fuse_candidate_for"] == 0
        assert g.kf_state(cur)["connection_updates"] == 0
    finally:
        g.close(); twin.close()


@pytest.mark.parametrize("rig", [False, True], ids=["stereo", "fisheye_rig"])
def test_process_new_keyframe_through_the_class(hip_lib, rig):
    g = make_scene(rig)
    try:
        cur = g.cur
        slots = g.kf_matches(cur).copy()
        new = [int(j) for i, j in enumerate(slots) if j >= 0 and i % 2 == 0]   # the keyframe holds them, they do not know it yet
        new = list(dict.fromkeys(new))
        for j in new:
            g.unlink(cur, j, keep_match=True)
        # :320-339 slot by slot: the first slot of a point that does not know the keyframe adds the observation, every other slot
        # (a point that knows it already, or the second slot of a rig point) goes to mlpRecentAddedMapPoints
        in_kf = {int(j) for j in slots if j >= 0 and cur in [kf for kf, _, _ in g.mp_observations(int(j))]}
        known, fresh = [], []
        for j in slots:
            if j < 0 or g.mp_state(int(j))["bad"]:
                continue
            (known if int(j) in in_kf else fresh).append(int(j))
            in_kf.add(int(j))
        assert len(fresh) >= 40 and len(known) >= 40 and np.array_equal(g.kf_matches(cur), slots)
        before = [g.mp_refresh(j) for j in range(g.n_mp)]
        n_listed = sum(int(np.sum(g.kf_matches(k) >= 0)) for k in range(7))
        out = g.process_new_keyframe(cur)
        assert list(out["recent"]) == known and out["in_map"] == 1
        assert g.kf_state(cur)["connection_updates"] == 1
        assert sum(int(np.sum(g.kf_matches(k) >= 0)) for k in range(7)) == n_listed
        for j in range(g.n_mp):
            now = g.mp_refresh(j)
            n = fresh.count(j)
            assert now["desc_updates"] - before[j]["desc_updates"] == n and now["normal_updates"] - before[j]["normal_updates"] == n, j
            if n:
                rows = [r for kf, left, right in g.mp_observations(j) if kf == cur for r in (left, right) if r != -1]
                assert rows and all(slots[r] == j for r in rows), j                 # the observation names its slot
                mn.assert_point_is_refreshed(g, j, {6})
            else:
                assert np.array_equal(now["desc"], before[j]["desc"]) and all(now[k].tobytes() == before[j][k].tobytes() for k in KEYS), j
    finally:
        g.close()


def test_refresh_batch_counts_every_occurrence(hip_lib):
    """A list with a duplicate, a null and a bad point."""
    g = make_scene(True)
    try:
        before = [g.mp_refresh(j) for j in range(g.n_mp)]
        g.set_bad(mp=3)
        g.refresh_batch([0, 1, -1, 3, 1, 2])
        for j, n in ((0, 1), (1, 2), (2, 1), (3, 0), (4, 0)):
            now = g.mp_refresh(j)
            assert now["desc_updates"] - before[j]["desc_updates"] == n and now["normal_updates"] - before[j]["normal_updates"] == n
            if n and g.mp_observations(j):
                mn.assert_point_is_refreshed(g, j, {6})
    finally:
        g.close()
