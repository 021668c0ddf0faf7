"""osh_orb_bow_transform and ORB_SLAM3::ORBVocabulary::transform on the device against the numpy restatement of reference
Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259 (tests/bow_numpy.py): every output, stage outputs included, equal; doubles
as their bit patterns; no tolerance."""

import numpy as np
import pytest

import bow_numpy as bn
from orb_slam3_study_kr_amd import capi, host, orb, synth
from orb_slam3_study_kr_amd import synth_bow as sb
from orb_slam3_study_kr_amd import synth_stereo as ss

pytestmark = pytest.mark.gpu


def _check(m, vocab, tree, frames, levelsup, what):
    got = m.bow_transform(vocab, frames, levelsup, stages=True)
    assert len(got) == len(frames)
    for k, d in enumerate(frames):
        bn.assert_same(got[k], bn.transform(tree, d, levelsup), f"{what}[{k}]")
    return got


def _one(tree, frames, levelsup, what):
    with orb.BowVocab(tree) as vocab, orb.OrbMatcher(0) as m:
        return _check(m, vocab, tree, frames, levelsup, what)


def _mixed_features(tree, seed, n):
    """Half random, half near leaves of the tree."""
    rng = np.random.default_rng(seed)
    leaves = rng.choice(tree.word_nodes(), size=min(30, int(tree.is_leaf.sum())), replace=False)
    return np.concatenate([sb.random_features(seed, n - n // 2), sb.features_near(tree, seed + 1, leaves, n // 2, 25)])


@pytest.fixture(scope="module")
def tree_10_4():
    return sb.make_vocab(41, k=10, L=4, zero_weight_prob=0.05)


@pytest.fixture(scope="module")
def sparse_10_6():
    tree = sb.make_vocab(42, k=10, L=6, shallow_leaf_prob=0.8, zero_weight_prob=0.05)
    assert 1500 < tree.n < 6000         # about 3000 nodes
    return tree


@pytest.mark.parametrize("name", [c[0] for c in bn.CASES])
def test_committed_cases_equal_the_restatement(hip_lib, name):
    tree, desc, levelsup = bn.build_case(name)
    _one(tree, [desc], levelsup, name)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257, 2000])
def test_feature_counts(hip_lib, tree_10_4, n):
    _one(tree_10_4, [_mixed_features(tree_10_4, 100 + n, n)], 2, f"n={n}")


@pytest.mark.parametrize("k,L", [(1, 3), (2, 10), (9, 3), (10, 6), (16, 2), (17, 2), (20, 2)])
def test_branching_and_depth(hip_lib, sparse_10_6, k, L):
    tree = sparse_10_6 if (k, L) == (10, 6) else sb.make_vocab(50 + k, k=k, L=L)
    assert max(len(c) for c in tree.children()) == k
    _one(tree, [_mixed_features(tree, 60 + k, 150)], min(L, 4), f"k={k} L={L}")


def test_mixed_child_counts(hip_lib):
    tree = sb.make_vocab(71, k=20, L=3, child_counts=(1, 7, 20))
    assert {len(c) for c in tree.children() if c} == {1, 7, 20}
    _one(tree, [_mixed_features(tree, 72, 200)], 1, "child counts 1, 7, 20")


@pytest.mark.parametrize("levelsup", [0, 1, 3, 4, 6])      # L = 4: 0, 1, L - 1, 4 = L, L + 2
def test_levelsup(hip_lib, levelsup):
    tree = sb.make_vocab(73, k=4, L=4, shallow_leaf_prob=0.2)
    _one(tree, [_mixed_features(tree, 74, 130)], levelsup, f"levelsup={levelsup}")


@pytest.mark.parametrize("weighting", [sb.TF_IDF, sb.TF, sb.IDF, sb.BINARY])
def test_weightings_and_scorings(hip_lib, weighting):
    desc = sb.random_features(75, 160)
    with orb.OrbMatcher(0) as m:
        for scoring in (sb.L1_NORM, sb.CHI_SQUARE, sb.KL, sb.BHATTACHARYYA, sb.DOT_PRODUCT):
            tree = sb.make_vocab(76, k=3, L=2, weighting=weighting, scoring=scoring, zero_weight_prob=0.1)
            with orb.BowVocab(tree) as vocab:
                _check(m, vocab, tree, [desc], 1, f"weighting {weighting} scoring {scoring}")


def test_l2_norm_is_unsupported_at_creation(hip_lib):
    with pytest.raises(capi.OshError) as e:
        orb.BowVocab(sb.make_vocab(77, k=3, L=2, scoring=sb.L2_NORM))
    assert e.value.code == capi.OSH_ERR_UNSUPPORTED and "L2" in str(e.value)


def test_300_features_on_one_word(hip_lib, tree_10_4):
    one = sb.features_near(tree_10_4, 78, tree_10_4.word_nodes()[1234:1235], 1, 3)
    exp = bn.transform(tree_10_4, one, 2)
    assert len(exp["word_id"]) == 1                         # not a stopped word
    got = _one(tree_10_4, [np.repeat(one, 300, axis=0)], 2, "one word")[0]
    assert got["word_id"].tolist() == exp["word_id"].tolist() and got["node_feat"].tolist() == list(range(300))


def test_300_features_on_300_words(hip_lib, tree_10_4):
    pool = sb.random_features(79, 1200)
    out = bn.transform(tree_10_4, pool, 2)
    words, first = np.unique(out["feat_word"], return_index=True)       # the first feature of every word reached
    pick = np.sort(first[np.isin(words, out["word_id"])][:300])         # of the words that are not stopped
    got = _one(tree_10_4, [pool[pick]], 2, "own words")[0]
    assert len(pick) == 300 and len(got["word_id"]) == 300


def test_every_word_stopped(hip_lib):
    tree, desc, levelsup = bn.build_case("all_words_stopped")
    got = _one(tree, [desc], levelsup, "all stopped")[0]
    assert len(got["word_id"]) == len(got["word_value"]) == len(got["node_id"]) == len(got["node_feat"]) == 0
    assert got["node_start"].tolist() == [0] and len(got["feat_word"]) == len(desc)


def test_batch_equals_single_calls(hip_lib, tree_10_4):
    frames = [_mixed_features(tree_10_4, 80, 300), np.zeros((0, 32), np.uint8), sb.random_features(81, 1), _mixed_features(tree_10_4, 82, 65),
              sb.random_features(83, 1000), np.zeros((0, 32), np.uint8)]
    with orb.BowVocab(tree_10_4) as vocab, orb.OrbMatcher(0) as m:
        batch = _check(m, vocab, tree_10_4, frames, 2, "batch")
        assert m.bow_transform(vocab, [], 2) == []                    # n_frames = 0 is OSH_OK
        for k, d in enumerate(frames):
            bn.assert_same(m.bow_transform(vocab, [d], 2, stages=True)[0], batch[k], f"single[{k}]")
        for k, o in enumerate(m.bow_transform(vocab, frames, 2)):    # without the stage outputs (they then stay on the device)
            bn.assert_same(o, batch[k], f"no stages[{k}]", stages=False)


def test_two_vocabularies_alternate_on_one_context(hip_lib, tree_10_4):
    other = sb.make_vocab(84, k=17, L=2, weighting=sb.TF, scoring=sb.DOT_PRODUCT)
    d1, d2 = _mixed_features(tree_10_4, 85, 200), _mixed_features(other, 86, 90)
    with orb.BowVocab(tree_10_4) as v1, orb.BowVocab(other) as v2, orb.OrbMatcher(0) as m:
        for _ in range(2):
            _check(m, v1, tree_10_4, [d1], 2, "first vocabulary")
            _check(m, v2, other, [d2, d2[:7]], 1, "second vocabulary")


def test_one_vocabulary_on_two_contexts(hip_lib, tree_10_4):
    d1, d2 = _mixed_features(tree_10_4, 87, 120), _mixed_features(tree_10_4, 88, 333)
    with orb.BowVocab(tree_10_4) as vocab, orb.OrbMatcher(0) as m1, orb.OrbMatcher(0) as m2:
        a = _check(m1, vocab, tree_10_4, [d1], 2, "context 1")
        _check(m2, vocab, tree_10_4, [d2], 2, "context 2")
        bn.assert_same(_check(m2, vocab, tree_10_4, [d1], 2, "context 2 again")[0], a[0], "contexts")
        _check(m1, vocab, tree_10_4, [d2, d1], 2, "context 1 again")


def test_transform_does_not_depend_on_what_the_context_ran_before(hip_lib, tree_10_4):
    d = _mixed_features(tree_10_4, 89, 500)
    with orb.BowVocab(tree_10_4) as vocab:
        with orb.OrbMatcher(0) as fresh:
            exp = _check(fresh, vocab, tree_10_4, [d], 2, "fresh")[0]
        with orb.OrbMatcher(0) as used:
            used.stereo_match([ss.make_stereo_frame(90, n_left=600)])
            used.search([synth.make_orb_pair(91, 300, 300)])
            got = used.bow_transform(vocab, [d], 2, stages=True)[0]
            bn.assert_same(got, exp, "after a stereo match and a search")


def test_feature_count_limit(hip_lib):
    tree = sb.make_vocab(92, k=4, L=2)
    at_limit = sb.random_features(93, capi.OSH_BOW_MAX_FEATURES)
    past = np.concatenate([at_limit, at_limit[:1]])
    with orb.BowVocab(tree) as vocab, orb.OrbMatcher(0) as m:
        _check(m, vocab, tree, [at_limit], 1, "16384 features")
        with pytest.raises(capi.OshError) as e:
            m.bow_transform(vocab, [at_limit[:5], past], 1)
        assert e.value.code == capi.OSH_ERR_UNSUPPORTED
        _check(m, vocab, tree, [at_limit[:100]], 1, "after the refusal")


def _as_fv(out):
    return out["node_id"], out["node_start"], out["node_feat"]


@pytest.mark.parametrize("keyframe", [False, True])
def test_compute_bow_through_the_class(hip_lib, sparse_10_6, tmp_path, keyframe):
    sb.write_text(sparse_10_6, tmp_path / "voc.txt")
    d = _mixed_features(sparse_10_6, 94, 400)
    exp = bn.transform(sparse_10_6, d, 4)
    with host.HostBowVocab(tmp_path / "voc.txt") as voc:
        assert voc.loaded
        bn.assert_same(voc.compute_bow(d, keyframe), exp, "ComputeBoW", stages=False)
        # the guard: a second call on other descriptors leaves the vectors as they are
        bn.assert_same(voc.compute_bow(d, keyframe, second_desc=sb.random_features(95, 400)), exp, "second call", stages=False)
        # several threads at once on one vocabulary, each with the matcher context of its thread
        bn.assert_same(voc.compute_bow(d, keyframe, n_threads=3), exp, "three threads", stages=False)
        empty = voc.compute_bow(np.zeros((0, 32), np.uint8), keyframe)
        assert len(empty["word_id"]) == 0 and len(empty["node_id"]) == 0


def test_search_by_bow_on_the_computed_feature_vectors(hip_lib, sparse_10_6, tmp_path):
    sb.write_text(sparse_10_6, tmp_path / "voc.txt")
    p = synth.make_bow_pair(96, n_kf=500, n_f=550, flip=0.01)
    has2 = np.ones(len(p["f_desc"]), np.uint8)
    with host.HostBowVocab(tmp_path / "voc.txt") as voc:
        fv1, fv2 = _as_fv(voc.compute_bow(p["kf_desc"], True)), _as_fv(voc.compute_bow(p["f_desc"], True))
    ref1, ref2 = _as_fv(bn.transform(sparse_10_6, p["kf_desc"], 4)), _as_fv(bn.transform(sparse_10_6, p["f_desc"], 4))
    n, m = host.search_by_bow_keyframes(p["kf_desc"], p["kf_angle"], p["kf_has_mp"], fv1, p["f_desc"], p["f_angle"], has2, fv2)
    n_ref, m_ref = host.search_by_bow_keyframes(p["kf_desc"], p["kf_angle"], p["kf_has_mp"], ref1, p["f_desc"], p["f_angle"], has2, ref2)
    assert n == n_ref and n > 0
    assert np.array_equal(m, m_ref)
