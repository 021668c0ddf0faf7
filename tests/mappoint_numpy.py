"""MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth restated from their definitions (include/orbslam3_hip.h,
"map point refresh") with np.sort, the first argmin and a float32 chain: the reference of test_mappoint_refresh_cpu.py and
test_gpu_mappoint_refresh.py.  Nothing here shares code with csrc/mappoint_refresh.h."""
from __future__ import annotations

import functools

import numpy as np

from orb_slam3_study_kr_amd import synth_mappoints as sm

F = np.float32
_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming_table(desc: np.ndarray) -> np.ndarray:
    """[M, M] Hamming distances of M 32-byte descriptors."""
    return _POPCOUNT[desc[:, None, :] ^ desc[None, :, :]].sum(axis=2)


def norm3(v: np.ndarray) -> np.ndarray:
    """sqrt(x*x + (y*y + z*z)) in float32 for rows of v."""
    sq = v * v
    return np.sqrt(sq[..., 0] + (sq[..., 1] + sq[..., 2]))


def refresh_point(desc, centre, use_desc, centres, pos, ref_centre, level_scale, top_scale):
    """One point: (best_entry, best_median, normal[3], min_distance, max_distance)."""
    n = int(desc.shape[0])
    if n == 0:
        return -1, -1, np.zeros(3, F), F(0), F(0)
    used = np.flatnonzero(use_desc)
    best_entry = best_median = -1
    if used.size:
        rows = np.sort(hamming_table(desc[used]), axis=1)            # ascending rows, self-distance included
        medians = rows[:, (used.size - 1) // 2]
        first = int(np.argmin(medians))                              # the first of the least
        best_entry, best_median = int(used[first]), int(medians[first])
    pos = np.asarray(pos, F)
    normali = pos[None, :] - centres[centre]                         # float32 throughout
    unit = normali / norm3(normali)[:, None]
    normal = np.zeros(3, F)
    for u in unit:                                                   # one chain in entry order
        normal = normal + u
    normal = normal / F(n)
    dist = norm3(pos - centres[ref_centre])
    max_distance = F(dist * F(level_scale))
    min_distance = F(max_distance / F(top_scale))
    return best_entry, best_median, normal.astype(F), min_distance, max_distance


def refresh_batch(b) -> dict:
    """A synth_mappoints.Batch: the dict OrbMatcher.refresh_map_points returns for it."""
    P = b.n_points
    out = dict(best_entry=np.zeros(P, np.int32), best_median=np.zeros(P, np.int32), normal=np.zeros((P, 3), F),
               min_distance=np.zeros(P, F), max_distance=np.zeros(P, F))
    centres = np.asarray(b.centres, F).reshape(-1, 3)
    for p in range(P):
        e0, e1 = int(b.entry_off[p]), int(b.entry_off[p + 1])
        r = refresh_point(b.desc[e0:e1], b.centre[e0:e1], b.use_desc[e0:e1], centres, b.pos[p], int(b.ref_centre[p]) if e1 > e0 else 0,
                          b.level_scale[p], b.top_scale[p])
        out["best_entry"][p], out["best_median"][p], out["normal"][p], out["min_distance"][p], out["max_distance"][p] = r
    return out


LIMIT = 256   # OSH_MAPPOINT_MAX_DESCRIPTORS
# entries per point: the median index at its small values, the wavefront edge, the switch to the block class, the limit
COUNTS = (1, 2, 3, 4, 5, 63, 64, 65, 128, LIMIT)


@functools.lru_cache(maxsize=None)
def generator_case(seed: int, n_points: int = 300):
    """A batch from the generator's distribution and its restatement (computed once, shared, not to be written to)."""
    b = sm.make_batch(seed, n_points)
    return b, refresh_batch(b)


@functools.lru_cache(maxsize=None)
def shapes_case():
    """One point of every count of COUNTS, each twice (two seeds of descriptors), and points without entries between them."""
    counts = []
    for n in COUNTS:
        counts += [n, 0, n]
    b = sm.make_batch(11, counts=counts)
    return b, refresh_batch(b)


@functools.lru_cache(maxsize=None)
def special_case():
    """Hand-made points, by name -> index in the batch:
      unused      entries whose use_desc are all 0: the normal is computed, best_entry is -1
      empty       no entries
      identical   all descriptors identical: every median is 0, entry 0 wins
      tie         two rows share the least median: the lower index wins
      holes       use_desc 0 at the first and the last entry
      identical65 / unused65 / holes65: the same above a wavefront"""
    names = ["unused", "empty", "identical", "tie", "holes", "identical65", "unused65", "holes65"]
    counts = [9, 0, 12, 7, 17, 65, 65, 65]
    b = sm.make_batch(12, counts=counts, bad_fraction=0.0)
    at = {n: i for i, n in enumerate(names)}
    rng = np.random.default_rng(13)
    for name in ("unused", "unused65"):
        b = sm.edit_point(b, at[name], use_desc=np.zeros(counts[at[name]], np.uint8))
    for name in ("identical", "identical65"):
        b = sm.edit_point(b, at[name], desc=np.tile(rng.integers(0, 256, 32, dtype=np.uint8), (counts[at[name]], 1)))
    # tie: rows 1 and 3 are the same descriptor c, rows 0, 2, 4, 5, 6 differ from c in 40 disjoint bits each (80 from one
    # another): sorted rows 1 and 3 are [0, 0, 40 x 5] with median 40 at index 3, the others [0, 40, 40, 80 x 4] with median 80
    c = np.unpackbits(rng.integers(0, 256, 32, dtype=np.uint8))
    rows = np.tile(c, (7, 1))
    for k, r in enumerate((0, 2, 4, 5, 6)):
        rows[r, 40 * k:40 * (k + 1)] ^= 1
    b = sm.edit_point(b, at["tie"], desc=np.packbits(rows, axis=1))
    for name in ("holes", "holes65"):
        use = np.ones(counts[at[name]], np.uint8)
        use[0] = use[-1] = 0
        b = sm.edit_point(b, at[name], use_desc=use)
    return b, refresh_batch(b), at


def restate_graph_point(g, j, bad_kfs=()):
    """Point j from the observation graph the library exports, the descriptors and octaves the test handed in and the centres the
    keyframes report: the entries in exported order, a left and a right index of one keyframe as two entries, left first."""
    obs = g.mp_observations(j)
    st = g.mp_state(j)
    desc, centre, use, centres = [], [], [], []
    for kf, left, right in obs:
        c = g.kf_state(kf)["centres"]
        for cam, row in ((0, left), (1, right)):
            if row == -1:
                continue
            desc.append(g.kf_desc[kf][row]); use.append(0 if kf in bad_kfs else 1)
            centre.append(len(centres)); centres.append(c[cam])
    ref = st["ref_kf"]
    by_kf = {kf: (left, right) for kf, left, right in obs}
    left, right = by_kf.get(ref, (0, 0))                        # std::map::operator[] default-constructs (0, 0)
    n_left = g.kf_state(ref)["n_left"]
    level = g.kf_octave[ref][left] if (n_left == -1 or left != -1) else g.kf_octave[ref][right]
    centres.append(g.kf_state(ref)["centres"][0])
    return refresh_point(np.array(desc, np.uint8).reshape(-1, 32), np.array(centre, np.int64), np.array(use, np.uint8),
                            np.array(centres, F).reshape(-1, 3), g.mp_pos(j), len(centres) - 1, g.scale_factors[level], g.scale_factors[-1])


def assert_point_is_refreshed(g, j, bad_kfs=()):
    """Descriptor, normal and distances of point j equal the restatement on the observation graph as it is now."""
    e = restate_graph_point(g, j, bad_kfs)
    got = g.mp_refresh(j)
    assert got["has_desc"], j
    flat = [(kf, r) for kf, left, right in g.mp_observations(j) for r in (left, right) if r != -1]
    kf, row = flat[e[0]]
    assert np.array_equal(got["desc"], g.kf_desc[kf][row]), j
    assert np.array_equal(got["normal"].view(np.uint32), e[2].view(np.uint32)), j
    assert got["min_distance"].tobytes() == e[3].tobytes() and got["max_distance"].tobytes() == e[4].tobytes(), j


def same_bits(a: dict, b: dict, names=None) -> list:
    """The names of the outputs that differ in any bit."""
    return [k for k in (names or a) if not np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8))]
