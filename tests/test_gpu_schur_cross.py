"""Cross items of the Schur plan (parts a < b of tracks with 9-13 optimisable observers, csrc/lba_schur_items.h:k_schur_fused<false, false>):
the column side of an item with at most four column poses is formed for two chunks of 8 landmarks in one 16 x 4 pass.  Windows of 14
optimisable + 2 fixed keyframes whose landmarks are all seen by 9-13 optimisable keyframes, so that the cross items carry every block
of S they touch; each window is checked to contain the chunk shapes it is named after (a Python restatement of the cross-item part of
csrc/schur_plan.h:plan_window, itself checked against the uploaded plan's item counts).  S and b_s of one trial against the CPU oracle
at the tolerances of tests/test_gpu_lba.py; the whole optimisation bit for bit against arrays recorded on the GPU with the build that
formed the column side per chunk (tests/golden/schur_cross_*.npz): the k sequence of every Schur product is unchanged, so its bits are."""
import dataclasses

import numpy as np
import pytest

from orb_slam3_study_kr_amd import lba, synth

pytestmark = pytest.mark.gpu

N_FREE, N_FIXED = 14, 2
LAMBDA = 1e-3

# name -> (landmarks per item at most, [(first observer o, observers k, landmarks n)]): the landmarks of a group are seen by the
# optimisable keyframes o .. o + k - 1 (and the two fixed ones).  Row poses o .. o + 7, column poses o + 8 .. o + k - 1; groups with
# different o have different row poses and are never merged into one item (the union would have 9).
CASES = {
    # one chunk per item: 5, 8, 1 and 7 landmarks; ny = 1, 2, 3, 4
    "one_chunk": (24, [(5, 9, 5), (4, 10, 8), (3, 11, 1), (2, 12, 7), (0, 9, 8), (1, 9, 3)]),
    # three chunks per item (an odd number: the last chunk has no partner): last chunk of 1, 7, 8 and 4 landmarks; ny = 1, 2, 3, 4
    "three_chunks": (24, [(5, 9, 17), (4, 10, 23), (3, 11, 24), (2, 12, 20), (0, 10, 19), (1, 9, 22)]),
    # two chunks (last of 1 and of 7), a group cut into items of 24 and 16 landmarks, and 13 observers: five column poses, the 8 x 8 column pass
    "two_chunks_and_five_columns": (24, [(5, 9, 9), (2, 12, 15), (3, 11, 40), (1, 13, 10), (0, 13, 21), (4, 10, 16)]),
    # the items of a large batch (64 landmarks at most): 8, 6 (last of 1) and 5 (last of 7) chunks -- more than one pair per item
    "long_items": (64, [(5, 9, 64), (2, 12, 41), (3, 11, 39), (4, 10, 50), (1, 13, 33)]),
}


def make_case(name):
    item_max, groups = CASES[name]
    base = synth.make_window(4100 + sorted(CASES).index(name), n_free=N_FREE, n_fixed=N_FIXED, n_points=1500, stereo=True,
                             track_len=(N_FREE + N_FIXED,) * 2, kf_spacing=0.05)
    full = np.nonzero(np.bincount(base.edge_point, minlength=base.n_points) == N_FREE + N_FIXED)[0]   # seen by every keyframe
    assert full.size >= sum(n for _, _, n in groups)
    keep = np.zeros(base.n_edges, dtype=bool)
    at = 0
    for o, k, n in groups:
        in_group = np.isin(base.edge_point, full[at:at + n])
        keep |= in_group & ((base.edge_pose >= N_FREE) | ((base.edge_pose >= o) & (base.edge_pose < o + k)))
        at += n
    lms = full[:at]
    remap = -np.ones(base.n_points, dtype=np.int64)
    remap[lms] = np.arange(at)
    w = dataclasses.replace(base, points=base.points[lms], edge_pose=base.edge_pose[keep], edge_point=remap[base.edge_point[keep]].astype(np.int32),
                            edge_kind=base.edge_kind[keep], edge_obs=base.edge_obs[keep], edge_info=base.edge_info[keep],
                            gt_points=None, outlier_mask=None)
    return w.normalise(), item_max


def cross_items(w, item_max):
    """(nx, ny, landmarks) of every cross item of window ``w``, in plan order: schur_plan.h:plan_window restricted to the part pairs a < b."""
    tiles_of = lambda n: (6 * n + 15) // 16
    obs = [[] for _ in range(w.n_points)]
    free = w.edge_pose < w.n_free
    for ip, il in zip(w.edge_pose[free].tolist(), w.edge_point[free].tolist()):
        obs[il].append(ip)
    units = []
    for j, o in enumerate(obs):
        o.sort()
        nparts = (len(o) + 7) // 8
        for a in range(nparts):
            for b in range(a + 1, nparts):
                X, Y = tuple(o[8 * a:8 * a + 8]), tuple(o[8 * b:8 * b + 8])
                units.append((X + (0xffff,) * (8 - len(X)) + Y + (0xffff,) * (8 - len(Y)), j, a, b, X, Y))
    units.sort(key=lambda u: u[:4])
    items, cur = [], None   # cur: [row poses, column poses, units]

    def flush():
        for base in range(0, cur[2], item_max):
            items.append((len(cur[0]), len(cur[1]), min(item_max, cur[2] - base)))

    x = 0
    while x < len(units):
        x1 = x + 1
        while x1 < len(units) and units[x1][0] == units[x][0]:
            x1 += 1
        gX, gY = set(units[x][4]), set(units[x][5])
        merged = False
        if cur is not None and cur[2] < item_max:
            ux, uy = cur[0] | gX, cur[1] | gY
            if (len(ux) <= 8 and len(uy) <= 8 and tiles_of(len(ux)) == tiles_of(len(cur[0])) == tiles_of(len(gX))
                    and tiles_of(len(uy)) == tiles_of(len(cur[1])) == tiles_of(len(gY))):
                cur[0], cur[1], merged = ux, uy, True
        if not merged:
            if cur is not None:
                flush()
            cur = [gX, gY, 0]
        cur[2] += x1 - x
        x = x1
    if cur is not None:
        flush()
    return items


def shapes(items):
    """{(ny, chunks, landmarks of the last chunk)} of a list of cross items"""
    return {(ny, (n + 7) // 8, (n - 1) % 8 + 1) for _, ny, n in items}


# what each window is there for: (ny, chunks, landmarks of the last chunk) of some of its cross items
EXPECTED = {
    "one_chunk": {(1, 1, 5), (2, 1, 8), (3, 1, 1), (4, 1, 7)},
    "three_chunks": {(1, 3, 1), (2, 3, 7), (3, 3, 8), (4, 3, 4)},
    "two_chunks_and_five_columns": {(1, 2, 1), (4, 2, 7), (3, 3, 8), (3, 2, 8), (5, 2, 2), (5, 3, 5)},
    "long_items": {(1, 8, 8), (4, 6, 1), (3, 5, 7), (2, 7, 2), (5, 5, 1)},
}


@pytest.fixture(scope="module")
def solver(hip_lib):
    with lba.LbaSolver(0) as s:
        yield s


@pytest.fixture(scope="module")
def ob():
    from oracle import binding
    return binding


def run_case(solver, name, monkeypatch):
    """The window of a case, uploaded alone; S, b_s of one trial and the result of optimize().  (Also what recorded the golden arrays.)"""
    w, item_max = make_case(name)
    monkeypatch.setenv("OSH_LBA_ITEM_MAX", str(item_max))   # 24 is what a single window gets anyway; 64: the items of a large batch
    solver.upload([w])
    st = solver.plan_stats()
    S, bs, _ = solver.debug_trial(0, LAMBDA)
    solver.optimize()
    return w, item_max, st, S, bs, solver.download()[0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_cross_items_match_the_oracle_and_keep_their_bits(solver, ob, golden_dir, monkeypatch, name):
    w, item_max, st, S, bs, got = run_case(solver, name, monkeypatch)
    # the window contains what it is named after, and the restated plan is the uploaded one
    k = np.bincount(w.edge_point[w.edge_pose < w.n_free], minlength=w.n_points)
    assert k.min() >= 9 and k.max() <= 13
    items = cross_items(w, item_max)
    assert st["items"] - st["sym_items"] == len(items)
    assert all(nx == 8 for nx, _, _ in items)
    assert EXPECTED[name] <= shapes(items), shapes(items)
    # one trial against the oracle (tolerances of tests/test_gpu_lba.py::test_observer_set_grouping_ragged_and_long_tracks)
    So, bso, _ = ob.lba_schur_step(w, LAMBDA)
    iu = np.triu_indices(S.shape[0])
    np.testing.assert_allclose(S[iu], So[iu], rtol=1e-10, atol=1e-11 * np.abs(So).max())
    np.testing.assert_allclose(bs, bso, rtol=1e-10, atol=1e-11 * np.abs(bso).max())
    # the same bits as the per-chunk column pass
    z = np.load(golden_dir / f"schur_cross_{name}.npz")
    np.testing.assert_array_equal(S[iu], z["S"][iu])
    np.testing.assert_array_equal(bs, z["bs"])
    assert got.iterations == int(z["iterations"]) and got.iterations > 0
    np.testing.assert_array_equal(got.trials_trace, z["trials_trace"])
    np.testing.assert_array_equal(got.chi2_trace, z["chi2_trace"])
    np.testing.assert_array_equal(got.lambda_trace, z["lambda_trace"])
    np.testing.assert_array_equal(got.pose_qt, z["pose_qt"])
    np.testing.assert_array_equal(got.points, z["points"])
