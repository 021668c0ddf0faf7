"""Synthetic DBoW2 vocabularies for the bag-of-words transform (osh_bow_tree of include/orbslam3_hip.h): random trees of a given
branching factor and depth with the irregularities a loaded vocabulary may show, features near chosen leaves, and the text format
of TemplatedVocabulary::loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1337-1424)."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

TF_IDF, TF, IDF, BINARY = range(4)
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)


@dataclass
class BowTree:
    """Nodes 1..n in file order; the root is node 0."""
    k: int
    L: int
    weighting: int
    scoring: int
    parent: np.ndarray    # [n] int32, parent of node i + 1
    is_leaf: np.ndarray   # [n] uint8
    desc: np.ndarray      # [n, 32] uint8
    weight: np.ndarray    # [n] float64

    @property
    def n(self) -> int:
        return int(self.parent.shape[0])

    def children(self) -> list[list[int]]:
        """Child node ids of every node 0..n in the order the loader appends them (file order)."""
        ch = [[] for _ in range(self.n + 1)]
        for i, p in enumerate(self.parent.tolist()):
            ch[p].append(i + 1)
        return ch

    def word_nodes(self) -> np.ndarray:
        """Node id of every word: words are numbered in file order over the nodes flagged leaf."""
        return (np.flatnonzero(self.is_leaf) + 1).astype(np.int32)


def make_vocab(seed: int, k: int, L: int, weighting: int = TF_IDF, scoring: int = L1_NORM, child_counts=None,
               shallow_leaf_prob: float = 0.0, dup_sibling_prob: float = 0.0, zero_weight_prob: float = 0.0,
               scatter_order: bool = False) -> BowTree:
    """A random tree.  child_counts: the numbers of children an inner node may get (default: always k; fewer than k children
    otherwise).  shallow_leaf_prob: a node above depth L becomes a leaf with this probability (the first child of a node never
    does, so the tree keeps its depth).  dup_sibling_prob: a node copies the descriptor of the sibling before it.
    zero_weight_prob: a word gets the weight 0 or -1 (a stopped word).  scatter_order: the file order keeps parents before
    children but not siblings next to each other."""
    rng = np.random.default_rng(seed)
    counts = [k] if child_counts is None else list(child_counts)
    parent, depth, leaf = [], [0], [False]          # by construction id; entry 0 of depth / leaf is the root
    frontier = [0]
    while frontier:
        nxt = []
        for p in frontier:
            for c in range(int(rng.choice(counts))):
                d = depth[p] + 1
                is_leaf = d >= L or (c > 0 and rng.random() < shallow_leaf_prob)
                parent.append(p); depth.append(d); leaf.append(is_leaf)
                if not is_leaf:
                    nxt.append(len(depth) - 1)
        frontier = nxt
    n = len(parent)
    desc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    prev_sibling = {}
    for i, p in enumerate(parent):
        if p in prev_sibling and rng.random() < dup_sibling_prob:
            desc[i] = desc[prev_sibling[p]]
        prev_sibling[p] = i
    weight = np.where(np.array(leaf[1:]), rng.uniform(0.05, 9.0, size=n), 0.0)
    stopped = np.array(leaf[1:]) & (rng.random(n) < zero_weight_prob)
    weight[stopped] = rng.choice([0.0, -1.0], size=int(stopped.sum()))
    order = np.arange(n)
    if scatter_order:                               # a random order among those in which every parent comes first
        ch = [[] for _ in range(n + 1)]
        for i, p in enumerate(parent):
            ch[p].append(i + 1)
        avail, out = list(ch[0]), []
        while avail:
            j = int(rng.integers(len(avail)))
            node = avail[j]
            avail[j] = avail[-1]; avail.pop()
            out.append(node)
            avail += ch[node]
        order = np.array(out) - 1
    new_id = np.zeros(n + 1, dtype=np.int64)
    new_id[order + 1] = np.arange(1, n + 1)
    return BowTree(k, L, weighting, scoring, new_id[np.array(parent, dtype=np.int64)[order]].astype(np.int32),
                   np.array(leaf[1:], dtype=np.uint8)[order], np.ascontiguousarray(desc[order]), np.ascontiguousarray(weight[order]))


def make_full_vocab(seed: int, k: int = 10, L: int = 6, weighting: int = TF_IDF, scoring: int = L1_NORM) -> BowTree:
    """The full k-way tree of depth L in breadth-first file order, without a Python loop over its nodes: k = 10, L = 6 has the
    1 111 110 nodes besides the root (10^6 words) of ORBvoc.txt."""
    rng = np.random.default_rng(seed)
    n = (k ** (L + 1) - k) // (k - 1)
    ids = np.arange(1, n + 1, dtype=np.int64)
    first_leaf = n - k ** L + 1
    leaf = ids >= first_leaf
    return BowTree(k, L, weighting, scoring, ((ids - 1) // k).astype(np.int32), leaf.astype(np.uint8),
                   rng.integers(0, 256, size=(n, 32), dtype=np.uint8), np.where(leaf, rng.uniform(0.05, 9.0, size=n), 0.0))


def random_features(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)


def features_near(tree: BowTree, seed: int, nodes, n: int, flips: int = 12) -> np.ndarray:
    """n descriptors, each the descriptor of one of `nodes` (node ids, taken in turn) with `flips` random bits flipped."""
    rng = np.random.default_rng(seed)
    nodes = np.asarray(nodes, dtype=np.int64)
    out = np.unpackbits(tree.desc[nodes[np.arange(n) % len(nodes)] - 1], axis=1)
    for i in range(n):
        out[i, rng.choice(256, size=flips, replace=False)] ^= 1
    return np.packbits(out, axis=1)


def write_text(tree: BowTree, path, trailing_newline: bool = True, blank_lines: int = 0) -> None:
    """The text file loadFromTextFile reads: `k L scoring weighting`, then `parent leaf d0 .. d31 weight` per node.  Weights carry
    17 significant digits, so the load is exact.  blank_lines: empty lines appended after the last node."""
    lines = [f"{tree.k} {tree.L} {tree.scoring} {tree.weighting}"]
    for i in range(tree.n):
        d = " ".join(str(int(b)) for b in tree.desc[i])
        lines.append(f"{int(tree.parent[i])} {int(tree.is_leaf[i])} {d} {float(tree.weight[i]):.17g}")
    text = "\n".join(lines) + ("\n" if trailing_newline else "") + "\n" * blank_lines
    with open(path, "w") as f:
        f.write(text)
