"""Synthetic inputs for the keyframe database (osh_bow_db, ORB_SLAM3::KeyFrameDatabase): BowVectors over a word-id space, stand-in
keyframe graphs with scripts of operations, and the trajectory-like databases of profiles/kfdb_timing.py."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

ADD, ERASE, CLEAR_MAP, CLEAR, NBEST, RELOC = range(6)   # OSH_HOST_KFDB_* (include/orbslam3_hip_host.h)


def bow_vector(rng, n_words: int, n: int, pool=None):
    """n distinct ascending word ids (from `pool` if given) with positive values of L1 norm 1, as BowVector::normalize leaves them."""
    ids = np.sort(rng.choice(n_words if pool is None else pool, size=n, replace=False)).astype(np.int32)
    v = rng.random(n) + 0.05
    return ids, (v / np.sum(v)).astype(np.float64)


@dataclass
class KfdbGraph:
    """The flat description of a stand-in graph (osh_host_kfdb_graph): per keyframe mnId, map index, bad flag, BowVector, ordered
    covisibles and connected set; per map its bad flag; frames as (mnId, word ids, values)."""

    n_words: int
    kf_id: list
    kf_map: list
    kf_bad: list
    bow: list            # (word ids, values) per keyframe
    cov: list            # per keyframe the indices of mvpOrderedConnectedKeyFrames
    con: list            # per keyframe the indices of its connected keyframes
    map_bad: list
    frames: list = field(default_factory=list)   # (mnId, word ids, values)

    @property
    def n_kf(self):
        return len(self.kf_id)


def make_graph(seed: int, n_kf: int = 28, n_words: int = 48, n_maps: int = 3, max_len: int = 22, p_bad: float = 0.12,
               n_frames: int = 4, max_cov: int = 13) -> KfdbGraph:
    """A small graph on a small vocabulary, so that most keyframes share words: keyframes of one map draw their words from a pool
    of their neighbourhood, the last map is bad, a few keyframes have an empty BowVector."""
    rng = np.random.default_rng(seed)
    kf_map = [int(rng.integers(0, n_maps)) for _ in range(n_kf)]
    bow = []
    for k in range(n_kf):
        if rng.random() < 0.06:
            bow.append((np.zeros(0, np.int32), np.zeros(0, np.float64)))
            continue
        centre = int(rng.integers(0, n_words))
        pool = np.unique((centre + rng.integers(-n_words // 3, n_words // 3 + 1, size=4 * max_len)) % n_words)
        bow.append(bow_vector(rng, n_words, int(rng.integers(1, min(max_len, len(pool)) + 1)), pool))
    cov, con = [], []
    for k in range(n_kf):
        others = [j for j in range(n_kf) if j != k]
        c = [int(x) for x in rng.permutation(others)[:int(rng.integers(0, max_cov + 1))]]
        extra = [int(x) for x in rng.permutation(others)[:int(rng.integers(0, 3))]]
        keep = [j for j in c if rng.random() < 0.5]          # the connected set: some of the covisibles and a few others
        cov.append(c)
        con.append(sorted(set(keep + extra)))
    frames = []
    for f in range(n_frames):
        ids, v = bow_vector(rng, n_words, int(rng.integers(3, max_len + 1)))
        frames.append((0 if f == 0 else int(rng.integers(1, 6)), ids, v))   # ids repeat: a later frame meets stale markers
    return KfdbGraph(n_words, kf_id=[int(x) for x in rng.permutation(n_kf) + 1], kf_map=kf_map,
                     kf_bad=[int(rng.random() < p_bad) for _ in range(n_kf)], bow=bow, cov=cov, con=con,
                     map_bad=[0] * (n_maps - 1) + [1], frames=frames)


def make_script(seed: int, g: KfdbGraph, n_queries: int = 14) -> np.ndarray:
    """Adds most keyframes, then queries of both kinds (some repeated at once, so that markers are stale) mixed with erases, re-adds
    and one clearMap; at the end clear() and one query of each kind on the empty database."""
    rng = np.random.default_rng(seed + 7919)
    ops = []
    inside = []
    for k in rng.permutation(g.n_kf):
        if rng.random() < 0.85:
            ops.append((ADD, int(k), 0)); inside.append(int(k))
    cleared = False
    for q in range(n_queries):
        u = rng.random()
        if u < 0.55:
            k = int(rng.integers(0, g.n_kf))
            ops.append((NBEST, k, int(rng.integers(1, 4))))
            if rng.random() < 0.3:
                ops.append((NBEST, k, int(rng.integers(1, 6))))
        else:
            ops.append((RELOC, int(rng.integers(0, len(g.frames))), int(rng.integers(0, len(g.map_bad)))))
        v = rng.random()
        if q == n_queries // 2 and not cleared:
            v = 0.3                                          # every script has its clearMap
        elif q == 1:
            v = 0.0                                          # and an erase
        if v < 0.25 and inside:
            k = inside.pop(int(rng.integers(0, len(inside))))
            ops.append((ERASE, k, 0))
            if rng.random() < 0.5:
                ops.append((ADD, k, 0)); inside.append(k)
        elif v < 0.32 and not cleared:
            ops.append((CLEAR_MAP, 1, 0)); cleared = True
            inside = [k for k in inside if g.kf_map[k] != 1]
    ops += [(CLEAR, 0, 0), (NBEST, 0, 3), (RELOC, 0, 0)]
    return np.asarray(ops, dtype=np.int32)


def make_trajectory(seed: int, n_kf: int, n_words: int = 1_000_000, words_per_kf: int = 1200, window: int = 40, fresh: float = 0.12):
    """BowVectors of a camera moving through a scene: every keyframe keeps most words of its predecessor and replaces a share
    `fresh` of them by new ones, and now and then revisits the words of a keyframe `window` or more back.  Neighbours share many
    words, distant keyframes few.  Returns the list of (word ids, values)."""
    rng = np.random.default_rng(seed)
    cur = rng.choice(n_words, size=words_per_kf, replace=False)
    out, history = [], []
    for k in range(n_kf):
        if history and k % 97 == 96 and len(history) > window:        # a revisit
            cur = history[int(rng.integers(0, len(history) - window))].copy()
        n_new = int(round(fresh * words_per_kf))
        keep = rng.permutation(cur)[:words_per_kf - n_new]
        cur = np.unique(np.concatenate([keep, rng.integers(0, n_words, size=n_new)]))
        v = rng.random(len(cur)) + 0.05
        out.append((cur.astype(np.int32), (v / np.sum(v)).astype(np.float64)))
        history.append(cur)
    return out
