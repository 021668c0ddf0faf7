"""The bag-of-words transform without a device: the numpy restatement (tests/bow_numpy.py) against hand-computed answers, the
single-thread C++ restatement against it bit for bit, the text loader of ORB_SLAM3::ORBVocabulary, its refusals and score, and the
ctypes mirrors of the osh_bow_* structs."""
import ctypes as C
import re

import numpy as np
import pytest

import bow_numpy as bn
from orb_slam3_study_kr_amd import capi, host, orb
from orb_slam3_study_kr_amd import synth_bow as sb


def _hand_tree(weighting=sb.TF_IDF, scoring=sb.L1_NORM):
    """k = 2, L = 2.  Node 1 (inner, all 0x00) and node 2 (a leaf at depth 1, all 0xFF, word 0, weight 0.75) under the root; node 3
    (all 0x00, word 1, weight 1.5) and node 4 (two bytes 0xFF then zeros, word 2, weight 0: stopped) under node 1."""
    desc = np.zeros((4, 32), dtype=np.uint8)
    desc[1] = 0xFF
    desc[3, :2] = 0xFF
    return sb.BowTree(2, 2, weighting, scoring, np.array([0, 0, 1, 1], np.int32), np.array([0, 1, 1, 1], np.uint8), desc,
                      np.array([0.0, 0.75, 1.5, 0.0]))


def _hand_features():
    f = np.zeros((5, 32), dtype=np.uint8)
    f[1] = 0xFF          # the shallow leaf itself
    f[2, :16] = 0xFF     # 128 from node 1 and from node 2: the tie goes to node 1; then 128 from node 3, 112 from node 4: stopped
    f[3, 0] = 0xFF       # node 1; then 8 from node 3 and 8 from node 4: the tie goes to node 3
    return f             # features 0 and 4 are all zeros: node 1, node 3 at distance 0


HAND_WORD = [1, 0, 2, 1, 1]
HAND_DIST = [0, 0, 112, 8, 0]
# levelsup -> (feat_node, the FeatureVector): L - levelsup = 2, 1, 0, -1
HAND_NODES = {0: ([3, 2, 4, 3, 3], {2: [1], 3: [0, 3, 4]}),      # feature 1 stops at depth 1 and records its leaf
              1: ([1, 2, 1, 1, 1], {1: [0, 3, 4], 2: [1]}),
              2: ([0, 0, 0, 0, 0], {0: [0, 1, 3, 4]}),
              3: ([0, 0, 0, 0, 0], {0: [0, 1, 3, 4]})}


def _check_hand(out, levelsup):
    feat_node, fv = HAND_NODES[levelsup]
    assert out["feat_word"].tolist() == HAND_WORD and out["feat_dist"].tolist() == HAND_DIST
    assert out["feat_node"].tolist() == feat_node
    assert out["word_id"].tolist() == [0, 1]                       # word 2 is stopped: in neither vector
    norm = 0.75 + (1.5 + 1.5 + 1.5)
    assert out["word_value"].tolist() == [0.75 / norm, (1.5 + 1.5 + 1.5) / norm]
    assert out["node_id"].tolist() == sorted(fv)
    got = {int(a): out["node_feat"][out["node_start"][j]:out["node_start"][j + 1]].tolist() for j, a in enumerate(out["node_id"])}
    assert got == fv


@pytest.mark.parametrize("levelsup", [0, 1, 2, 3])
def test_hand_computed_tree(levelsup):
    tree, f = _hand_tree(), _hand_features()
    _check_hand(bn.transform(tree, f, levelsup), levelsup)
    _check_hand(host.bow_restatement(tree, f, levelsup), levelsup)


def test_hand_computed_weightings_and_scorings():
    f = _hand_features()
    for weighting, scoring, exp in [(sb.TF, sb.DOT_PRODUCT, [0.75 / 2.0, 4.5 / 2.0]), (sb.IDF, sb.DOT_PRODUCT, [0.75, 1.5]),
                                    (sb.BINARY, sb.KL, [0.75 / 2.25, 1.5 / 2.25]), (sb.TF_IDF, sb.BHATTACHARYYA, [0.75 / 5.25, 4.5 / 5.25])]:
        tree = _hand_tree(weighting, scoring)
        assert bn.transform(tree, f, 1)["word_value"].tolist() == exp
        assert host.bow_restatement(tree, f, 1)["word_value"].tolist() == exp


@pytest.fixture(scope="module")
def case_results():
    """name -> (tree, descriptors, levelsup, the numpy restatement's outputs, the branches it took)"""
    res = {}
    for name, *_ in bn.CASES:
        tree, desc, levelsup = bn.build_case(name)
        taken = set()
        res[name] = (tree, desc, levelsup, bn.transform(tree, desc, levelsup, taken), taken)
    return res


def test_cases_take_every_branch_and_show_the_order_of_the_sums(case_results):
    taken = set().union(*(r[4] for r in case_results.values()))
    assert taken == bn.BRANCHES, sorted(bn.BRANCHES - taken)
    # some word is hit three or more times and its sequential sum is not hits * weight
    sums = [s for name, (tree, _, _, out, _) in case_results.items() if tree.weighting in (sb.TF_IDF, sb.TF)
            for s in bn.raw_word_sums(tree, out)]
    assert any(hits >= 3 and total != hits * w for w, hits, total in sums)
    # the L1 norm of some case is not the same sum taken backwards
    differs = False
    for tree, _, _, out, _ in case_results.values():
        if tree.weighting not in (sb.TF_IDF, sb.TF) or tree.scoring == sb.DOT_PRODUCT:
            continue
        raw = [total for _, _, total in bn.raw_word_sums(tree, out)]
        fwd = bwd = 0.0
        for x in raw:
            fwd += x
        for x in reversed(raw):
            bwd += x
        differs |= fwd != bwd
    assert differs
    # the generator's options show in the trees
    ragged = case_results["ragged_shallow_leaves"][0]
    assert len({len(c) for c in ragged.children() if c}) > 1
    scattered = case_results["scattered_file_order"][0]
    assert any(np.any(np.diff(c) > 1) for c in scattered.children() if len(c) > 1) and np.all(scattered.parent <= np.arange(scattered.n))
    assert max(len(c) for c in case_results["wide_nodes"][0].children()) > 16


@pytest.mark.parametrize("name", [c[0] for c in bn.CASES])
def test_cpp_restatement_equals_numpy(case_results, name):
    tree, desc, levelsup, exp, _ = case_results[name]
    bn.assert_same(host.bow_restatement(tree, desc, levelsup), exp, name)


def test_text_file_round_trip(tmp_path):
    tree = sb.make_vocab(31, k=5, L=3, child_counts=(2, 5), shallow_leaf_prob=0.3, zero_weight_prob=0.2, scatter_order=True)
    words = tree.word_nodes()
    for name, kw in [("plain.txt", {}), ("no_newline.txt", dict(trailing_newline=False)), ("blank_lines.txt", dict(blank_lines=3))]:
        sb.write_text(tree, tmp_path / name, **kw)
        with host.HostBowVocab(tmp_path / name) as v:
            assert v.loaded
            got, getters, word_parent = v.tree(levelsup=1)
        assert got.n == tree.n, name                         # a trailing empty line adds no node
        assert (got.k, got.L, got.weighting, got.scoring) == (tree.k, tree.L, tree.weighting, tree.scoring)
        for field in ("parent", "is_leaf", "desc"):
            assert np.array_equal(getattr(got, field), getattr(tree, field)), field
        assert np.array_equal(got.weight.view(np.uint64), tree.weight.view(np.uint64))
        assert getters == dict(k=5, L=3, weighting=tree.weighting, scoring=tree.scoring, size=len(words), empty=False)
        assert word_parent.tolist() == [int(tree.parent[w - 1]) for w in words]   # getParentNode(w, 1)
    assert not host.HostBowVocab(tmp_path / "missing.txt").loaded
    (tmp_path / "header.txt").write_text("21 3 0 0\n0 1 " + "0 " * 32 + "1.0\n")
    assert not host.HostBowVocab(tmp_path / "header.txt").loaded


def _refused_trees():
    ok = _hand_tree()
    late_parent = _hand_tree()
    late_parent.parent = np.array([0, 0, 4, 1], np.int32)           # node 3 under node 4
    own_parent = _hand_tree()
    own_parent.parent = np.array([0, 0, 3, 1], np.int32)            # node 3 under itself
    leaf_with_child = _hand_tree()
    leaf_with_child.parent = np.array([0, 0, 2, 1], np.int32)       # node 3 under the leaf node 2
    inner_without_child = _hand_tree()
    inner_without_child.is_leaf = np.array([0, 1, 0, 1], np.uint8)  # node 3 flagged inner
    n = 21
    wide = sb.BowTree(20, 1, 0, 0, np.zeros(n, np.int32), np.ones(n, np.uint8), np.zeros((n, 32), np.uint8), np.ones(n))
    return ok, dict(late_parent=late_parent, own_parent=own_parent, leaf_with_child=leaf_with_child,
                    inner_without_child=inner_without_child, twenty_one_children=wide)


def test_refused_trees(tmp_path):
    lib = capi.load_library()
    ok, refused = _refused_trees()
    t, _keep = orb.bow_tree(ok)
    assert lib.osh_bow_tree_check(C.byref(t)) == capi.OSH_OK
    sb.write_text(ok, tmp_path / "ok.txt")
    assert host.HostBowVocab(tmp_path / "ok.txt").loaded
    for name, tree in refused.items():
        t, _keep = orb.bow_tree(tree)
        assert lib.osh_bow_tree_check(C.byref(t)) == capi.OSH_ERR_INVALID, name
        assert capi.last_error(lib), name
        sb.write_text(tree, tmp_path / f"{name}.txt")
        assert not host.HostBowVocab(tmp_path / f"{name}.txt").loaded, name
        with pytest.raises(RuntimeError):
            host.bow_restatement(tree, _hand_features(), 1)
    twenty = refused["twenty_one_children"]
    twenty = sb.BowTree(20, 1, 0, 0, twenty.parent[:20], twenty.is_leaf[:20], twenty.desc[:20], twenty.weight[:20])
    t, _keep = orb.bow_tree(twenty)
    assert lib.osh_bow_tree_check(C.byref(t)) == capi.OSH_OK          # twenty children are the limit


def _score(a: dict, b: dict) -> float:
    """L1Scoring::score in the reference's merge order: only the common words count."""
    s = 0.0
    for w in sorted(a):
        if w in b:
            s += abs(a[w] - b[w]) - abs(a[w]) - abs(b[w])
    return -s / 2.0


def test_score():
    rng = np.random.default_rng(5)
    def vec(ids):
        x = rng.uniform(0.01, 1.0, size=len(ids))
        return dict(zip(ids, (x / x.sum()).tolist()))
    a = vec(list(range(0, 60, 2)))
    pairs = dict(disjoint=(a, vec(list(range(1, 61, 2)))), identical=(a, dict(a)), overlapping=(a, vec(list(range(0, 90, 3)))),
                 empty=(a, {}))
    for name, (x, y) in pairs.items():
        got = host.bow_score(list(x), list(x.values()), list(y), list(y.values()))
        assert got == _score(x, y), name
    assert _score(*pairs["disjoint"]) == 0.0 and 0.0 < _score(*pairs["overlapping"]) < 1.0
    assert abs(_score(*pairs["identical"]) - 1.0) < 1e-12


def test_bow_structs_match_the_header_layout():
    assert C.sizeof(capi.BowTree) == 5 * 4 + 4 + 4 * 8
    assert [getattr(capi.BowTree, f).offset for f, _ in capi.BowTree._fields_] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    assert C.sizeof(capi.BowFrame) == 16 and capi.BowFrame.desc.offset == 8
    assert C.sizeof(capi.BowResult) == 10 * 8
    assert [getattr(capi.BowResult, f).offset for f, _ in capi.BowResult._fields_] == list(range(0, 80, 8))
    # the order of the fields is the header's
    header = (capi.REPO_ROOT / "include" / "orbslam3_hip.h").read_text()
    for struct, mirror in (("osh_bow_tree", capi.BowTree), ("osh_bow_frame", capi.BowFrame), ("osh_bow_result", capi.BowResult)):
        body = header.split(f"typedef struct {struct} {{")[1].split(f"}} {struct};")[0]
        pos = [re.search(rf"\b{name}\s*[;,]", body).start() for name, _ in mirror._fields_]
        assert pos == sorted(pos), struct
    assert (capi.OSH_BOW_MAX_K, capi.OSH_BOW_MAX_L, capi.OSH_BOW_MAX_FEATURES) == (20, 10, 16384)
