"""CPU checks of the keyframe database: the numpy restatement of the reference (tests/kfdb_numpy.py) pinned by hand-computed answers,
the branches its committed cases take, the C++ restatement of csrc/hosttest/kfdb.cc against it (candidates, markers, score bits),
the bookkeeping of osh_bow_db (csrc/bowdb_book.h) replayed against a model, and the refusals that need no device."""
import numpy as np
import pytest

import kfdb_numpy as kn
from orb_slam3_study_kr_amd import host
from orb_slam3_study_kr_amd import synth_bow as sb


@pytest.fixture(scope="module")
def case_runs():
    """Every committed case once: name -> (graph, script, numpy results, branches)."""
    runs = {}
    for name, _, _ in kn.CASES:
        g, ops = kn.build_case(name)
        runs[name] = (g, ops) + kn.run_script(g, ops)
    return runs


def test_hand_computed_answers():
    g, ops = kn.hand_case()
    (nbest, reloc), branches = kn.run_script(g, ops)
    # the query {0, 1, 2, 3} meets keyframes 0 and 2 at word 0 (add order breaks the tie), 1 and 3 at word 1; counts 3, 1, 3, 3;
    # min = (int)(3 * 0.8f) = 2, so 0, 1 and 3 are scored, each 0.75; 0 and 1 see each other: 1.5 each, the earlier one first
    assert nbest["loop"] == [0, 1] and nbest["merge"] == [3]
    assert nbest["marker"][:, :2].tolist() == [[9, 3], [9, 3], [9, 1], [9, 3], [0, 0]]
    assert nbest["score"][:, 0].tolist() == [0.75, 0.75, 0.0, 0.75, 0.0]
    # the frame {0: 0.75, 5: 0.25}: keyframe 0 shares one word, keyframe 2 two; min = (int)(2 * 0.8f) = 1: only 2 is scored,
    # -((|0.75 - 0.5| - 0.75 - 0.5) + (|0.25 - 0.5| - 0.25 - 0.5)) / 2 = 0.75
    assert reloc["loop"] == [2] and reloc["merge"] == []
    assert reloc["marker"][:, 2:].tolist() == [[7, 1], [0, 0], [7, 2], [0, 0], [0, 0]]
    assert reloc["score"][:, 1].tolist() == [0.0, 0.0, 0.75, 0.0, 0.0]
    assert {"first_word_tie", "loop_candidate", "merge_candidate", "count_equal_min_unscored"} <= branches


def test_hand_computed_device_rows():
    rows = [(1, [0, 1, 2], [0.5, 0.25, 0.25]), (2, [1, 2, 3, 4], [0.25] * 4), (3, [0, 5], [0.5, 0.5]), (4, [1, 2, 3], [0.5, 0.25, 0.25])]
    out = kn.db_query(rows, [0, 1, 2, 3], [0.25] * 4, excluded=[2])
    assert out == dict(max_common=3, min_common=2, handle=[1, 2, 3, 4], common=[3, 3, 1, 3], first_word=[0, 1, 0, 1], scored=[1, 0, 0, 1],
                       score=[0.75, 0.0, 0.0, 0.75])
    # an excluded row with the largest count does not set the maximum
    out = kn.db_query(rows, [1, 2, 3, 4], [0.25] * 4, excluded=[2])
    assert out["max_common"] == 3 and out["common"] == [2, 4, 3] and out["scored"] == [0, 0, 1]


def test_committed_cases_take_every_branch(case_runs):
    taken = set().union(*(r[3] for r in case_runs.values()))
    assert kn.BRANCHES - taken == set(), sorted(kn.BRANCHES - taken)
    assert taken <= kn.BRANCHES, sorted(taken - kn.BRANCHES)


def test_float_and_double_truncation_never_differ_below_the_word_limit():
    # the case "max_common * 0.8f where float and double truncation differ" does not exist: for every count a BowVector can reach,
    # (int)(m * 0.8f) in float, (int)(m * 0.8) in double and the exact floor(4 m / 5) agree, so the case is dropped
    m = np.arange(0, 16385)
    as_float = (m.astype(np.float32) * np.float32(0.8)).astype(np.int64)
    as_double = (m.astype(np.float64) * 0.8).astype(np.int64)
    assert np.array_equal(as_float, as_double) and np.array_equal(as_float, (4 * m) // 5)
    assert [kn.min_common(int(x)) for x in (0, 1, 4, 5, 6, 16384)] == [0, 0, 3, 4, 4, 13107]


def test_bit_equality_constrains_the_order_of_the_sum(case_runs):
    differ = total = 0
    for g, ops, _, _ in case_runs.values():
        for k in range(0, g.n_kf - 1, 3):
            a, b = g.bow[k], g.bow[k + 1]
            if len(kn.l1_terms(a[0], a[1], b[0], b[1])) >= 3:
                total += 1
                differ += kn.bits(kn.l1_score(a[0], a[1], b[0], b[1])) != kn.bits(kn.l1_score(a[0], a[1], b[0], b[1], reverse=True))
    assert total >= 20 and differ >= total // 4, (differ, total)


def test_l1_score_equals_the_host_score(case_runs):
    g = case_runs["dense"][0]
    for k in range(g.n_kf - 1):
        a, b = g.bow[k], g.bow[k + 1]
        assert kn.bits(host.bow_score(a[0], a[1], b[0], b[1])) == kn.bits(kn.l1_score(a[0], a[1], b[0], b[1]))


@pytest.mark.parametrize("name", [c[0] for c in kn.CASES] + ["hand"])
def test_cpp_restatement_equals_numpy(case_runs, name):
    g, ops = kn.hand_case() if name == "hand" else case_runs[name][:2]
    exp = kn.run_script(g, ops)[0] if name == "hand" else case_runs[name][2]
    got, ms = host.kfdb_restatement(g, ops)
    assert ms >= 0
    kn.assert_same_script(got, exp, name)


def _replay(ops):
    model, handles = kn.BookModel(), []
    for code, arg in ops:
        handles.append(model.add(arg) if code == 0 else 0)
        if code == 1:
            model.erase(arg)
        elif code == 2:
            model.clear()
    got = host.bowdb_book_replay(ops)
    assert got["op_handle"].tolist() == handles
    assert [list(r) for r in zip(got["handle"].tolist(), got["start"].tolist(), got["len"].tolist(), got["alive"].tolist())] == model.rows
    assert got["info"] == model.info()
    return got


def test_book_erase_then_add_again_takes_the_last_position():
    got = _replay([(0, 5), (0, 7), (0, 3), (1, 2), (0, 7)])
    assert got["handle"].tolist() == [1, 2, 3, 4] and got["alive"].tolist() == [1, 0, 1, 1] and got["start"].tolist() == [0, 5, 12, 15]
    assert got["info"]["compactions"] == 0 and got["info"]["live_rows"] == 3 and got["info"]["entries"] == 22


def test_book_compaction_trigger_and_order():
    # 10 + 10 + 10 + 10 entries; erasing two rows leaves the dead at exactly half: no compaction; a third erase finds 20 of 40
    # dead (not more than half) and then makes it 30: the next mutation compacts
    ops = [(0, 10)] * 4 + [(1, 1), (1, 3), (0, 0)]
    got = _replay(ops)
    assert got["info"]["compactions"] == 0 and got["handle"].tolist() == [1, 2, 3, 4, 5]
    got = _replay(ops + [(1, 2), (0, 4)])
    assert got["info"]["compactions"] == 1 and got["info"]["moved"] == 10
    assert got["handle"].tolist() == [4, 5, 6] and got["start"].tolist() == [0, 10, 10] and got["len"].tolist() == [10, 0, 4]
    assert got["info"]["entries"] == 14 and got["alive"].tolist() == [1, 1, 1]


def test_book_growth():
    first = kn.BookModel.FIRST_ENTRIES
    got = _replay([(0, 16384)] * (first // 16384) + [(0, 1)] + [(0, 16384)] * (first // 16384))
    assert got["info"]["capacity"] == 4 * first and got["info"]["reallocations"] == 4     # three arena sizes and the row table
    assert got["info"]["moved"] == 3 * first + 1 - 16384
    got = _replay([(0, 1)] * 2049)
    assert got["info"]["row_capacity"] == 4096 and got["info"]["rows"] == 2049


def test_book_random_scripts():
    rng = np.random.default_rng(5)
    ops, live, nxt = [], [], 1
    for _ in range(3000):
        u = rng.random()
        if u < 0.002:
            ops.append((2, 0)); live = []
        elif u < 0.45 and live:
            ops.append((1, live.pop(int(rng.integers(0, len(live))))))
        else:
            ops.append((0, int(rng.integers(0, 900)))); live.append(nxt); nxt += 1
    got = _replay(ops)
    assert got["info"]["compactions"] > 3


def test_word_lists_that_are_refused():
    assert host.bowdb_check_words([0, 3, 4, 9], 10) == 0 and host.bowdb_check_words([], 10) == 0
    assert host.bowdb_check_words([3, 1], 10) == 1          # unsorted
    assert host.bowdb_check_words([1, 2, 2], 10) == 1       # duplicate
    assert host.bowdb_check_words([1, 10], 10) == 2         # at the vocabulary size
    assert host.bowdb_check_words([-1, 2], 10) == 2


def test_a_vocabulary_that_is_not_l1_is_refused(tmp_path, capfd):
    # refused at construction: the class never reaches the device, finds nothing and touches no marker
    g, ops = kn.hand_case()
    sb.write_text(sb.make_vocab(3, k=3, L=2, scoring=sb.DOT_PRODUCT), tmp_path / "voc.txt")
    with host.HostBowVocab(tmp_path / "voc.txt") as voc:
        got, _ = host.kfdb_run(voc, g, ops)
    assert "L1_NORM" in capfd.readouterr().err
    assert len(got) == 2
    for q in got:
        assert q["loop"] == [] and q["merge"] == [] and not q["marker"].any() and not q["score"].any()
