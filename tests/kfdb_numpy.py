"""The reference's KeyFrameDatabase (src/KeyFrameDatabase.cc:32-98, 604-845) and L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) restated on Python ints and floats (IEEE doubles), with numpy.float32 wherever the
reference holds a float, and a literal list-per-word inverted file.  Every case records which branches it takes.  Beside it: the
model of one osh_orb_bow_db_query (what the device returns for a query against rows in add order) and of the bookkeeping of
csrc/bowdb_book.h.  The committed cases are graphs and scripts generated from seeds (orb_slam3_study_kr_amd/synth_kfdb.py) and a
few written by hand."""
import numpy as np

from orb_slam3_study_kr_amd import synth_kfdb as sk

F32 = np.float32


def l1_terms(qw, qv, rw, rv):
    """The terms of the reference's merge loop over the shared words, ascending: (|v - w| - |v|) - |w| with v of the query."""
    terms, i, j = [], 0, 0
    while i < len(qw) and j < len(rw):
        if qw[i] == rw[j]:
            vi, wi = float(qv[i]), float(rv[j])
            terms.append(abs(vi - wi) - abs(vi) - abs(wi))
            i += 1; j += 1
        elif qw[i] < rw[j]:
            i += 1
        else:
            j += 1
    return terms


def l1_score(qw, qv, rw, rv, reverse=False) -> float:
    s = 0.0
    for t in (reversed(l1_terms(qw, qv, rw, rv)) if reverse else l1_terms(qw, qv, rw, rv)):
        s += t
    return -s / 2.0


def min_common(max_common: int) -> int:
    """int minCommonWords = maxCommonWords*0.8f (:648): one float multiply, then truncation."""
    return int(F32(max_common) * F32(0.8))


def bits(x) -> int:
    return int(np.asarray(x, np.float64).view(np.uint64))


# ---------------------------------------------------------------- the C-ABI query

def db_query(rows, qw, qv, excluded=()):
    """What osh_orb_bow_db_query returns.  rows: the live rows in add order as (handle, word ids, values)."""
    qw = np.asarray(qw, np.int64)
    excluded = set(int(h) for h in excluded)
    listed = []
    for h, rw, rv in rows:
        shared = np.intersect1d(qw, np.asarray(rw, np.int64))
        if len(shared):
            listed.append((int(h), len(shared), int(shared[0]), rw, rv))
    max_c = max([c for h, c, _, _, _ in listed if h not in excluded], default=0)
    min_c = min_common(max_c)
    out = dict(max_common=max_c, min_common=min_c, handle=[], common=[], first_word=[], scored=[], score=[])
    for h, c, first, rw, rv in listed:
        scored = h not in excluded and c > min_c
        out["handle"].append(h); out["common"].append(c); out["first_word"].append(first); out["scored"].append(int(scored))
        out["score"].append(l1_score(qw, qv, rw, rv) if scored else 0.0)
    return out


def assert_same_query(got: dict, exp: dict, what: str):
    assert got["max_common"] == exp["max_common"] and got["min_common"] == exp["min_common"], (what, got["max_common"], got["min_common"], exp["max_common"], exp["min_common"])
    for k in ("handle", "common", "first_word", "scored"):
        assert [int(x) for x in got[k]] == [int(x) for x in exp[k]], (what, k)
    assert [bits(x) for x in got["score"]] == [bits(x) for x in exp["score"]], (what, "score bits")


# ---------------------------------------------------------------- the bookkeeping

class BookModel:
    """csrc/bowdb_book.h: rows as [handle, start, len, alive] in add order."""

    FIRST_ROWS, FIRST_ENTRIES = 1024, 1 << 18

    def __init__(self):
        self.rows, self.next_handle = [], 1
        self.entries = self.dead = self.row_cap = self.entry_cap = self.compactions = self.reallocations = self.moved = 0

    @staticmethod
    def _grown(cap, need, first):
        if need <= cap:
            return cap
        c = max(cap, first)
        while c < need:
            c *= 2
        return c

    def _prepare(self, extra, extra_rows):
        compacted = self.dead * 2 > self.entries
        if compacted:
            at, kept = 0, []
            for h, start, n, alive in self.rows:
                if alive:
                    kept.append([h, at, n, 1]); at += n
            self.rows, self.entries, self.dead = kept, at, 0
            self.compactions += 1
            self.moved += at
        cap = self._grown(self.entry_cap, self.entries + extra, self.FIRST_ENTRIES)
        if cap != self.entry_cap:
            if not compacted:
                self.moved += self.entries
            self.entry_cap = cap; self.reallocations += 1
        rows = self._grown(self.row_cap, len(self.rows) + extra_rows, self.FIRST_ROWS)
        if rows != self.row_cap:
            self.row_cap = rows; self.reallocations += 1

    def add(self, n):
        self._prepare(n, 1)
        self.rows.append([self.next_handle, self.entries, n, 1])
        self.entries += n
        self.next_handle += 1
        return self.next_handle - 1

    def erase(self, handle):
        self._prepare(0, 0)
        r = next(r for r in self.rows if r[0] == handle and r[3])
        r[3] = 0
        self.dead += r[2]

    def clear(self):
        self.rows, self.entries, self.dead = [], 0, 0

    def info(self):
        return dict(live_rows=sum(r[3] for r in self.rows), rows=len(self.rows), entries=self.entries, capacity=self.entry_cap,
                    compactions=self.compactions, reallocations=self.reallocations, row_capacity=self.row_cap, moved=self.moved)


# ---------------------------------------------------------------- the class

class _Kf:
    def __init__(self, g, k):
        self.index, self.id, self.map, self.bad = k, int(g.kf_id[k]), int(g.kf_map[k]), bool(g.kf_bad[k])
        self.words, self.values = [int(w) for w in g.bow[k][0]], [float(v) for v in g.bow[k][1]]
        self.cov, self.con = list(g.cov[k]), set(g.con[k])
        self.pr_query, self.pr_words, self.pr_score = 0, 0, F32(0)
        self.rl_query, self.rl_words, self.rl_score = 0, 0, F32(0)


class Reference:
    """The reference's class on a synth_kfdb.KfdbGraph; `branches` collects the names of the branches taken."""

    def __init__(self, g):
        self.g = g
        self.kf = [_Kf(g, k) for k in range(g.n_kf)]
        self.inverted = [[] for _ in range(g.n_words)]
        self.branches = set()

    def add(self, k):
        for w in self.kf[k].words:
            self.inverted[w].append(k)

    def erase(self, k):
        for w in self.kf[k].words:
            if k in self.inverted[w]:
                self.inverted[w].remove(k)          # the first, as :57-64

    def clear(self):
        self.inverted = [[] for _ in range(self.g.n_words)]

    def clear_map(self, m):
        for lst in self.inverted:
            lst[:] = [k for k in lst if self.kf[k].map != m]

    def _accumulate(self, scored, query_id, q_attr, s_attr, scored_now):
        acc_list, best_acc = [], F32(0)
        for si, k in scored:
            best_score, acc, best = si, si, k
            for k2 in self.kf[k].cov[:10]:
                n = self.kf[k2]
                if getattr(n, q_attr) != query_id:
                    continue
                s2 = getattr(n, s_attr)
                if k2 not in scored_now and float(s2) != 0.0:
                    self.branches.add("neighbour_listed_unscored_stale_score")
                acc = F32(acc + s2)
                if s2 > best_score:
                    best, best_score = k2, s2
                    self.branches.add("neighbour_becomes_best")
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return acc_list, best_acc

    def nbest(self, k, n_candidates):
        q = self.kf[k]
        sharing = []
        for w in q.words:
            lst = self.inverted[w]
            fresh = [i for i in lst if self.kf[i].pr_query != q.id and i not in q.con and i not in sharing]
            if len(fresh) > 1:
                self.branches.add("first_word_tie")
            for i in lst:
                kf = self.kf[i]
                if kf.pr_query != q.id:
                    kf.pr_words = 0
                    if i not in q.con:
                        kf.pr_query = q.id
                        sharing.append(i)
                    else:
                        self.branches.add("connected_not_listed")
                else:
                    if i not in sharing:
                        self.branches.add("stale_marker_nbest")
                kf.pr_words += 1
        if not sharing:
            self.branches.add("nbest_nothing_shared")
            return [], []
        max_c = max(self.kf[i].pr_words for i in sharing)
        # a connected keyframe shares more words than any listed one and must not set the maximum (its own count was reset)
        if any(len(set(q.words) & set(self.kf[i].words)) > max_c for i in q.con if any(i in self.inverted[w] for w in q.words)):
            self.branches.add("connected_has_largest_count")
        min_c = min_common(max_c)
        scored = []
        for i in sharing:
            kf = self.kf[i]
            if kf.pr_words > min_c:
                if kf.pr_words == min_c + 1:
                    self.branches.add("count_one_above_min")
                si = F32(l1_score(q.words, q.values, kf.words, kf.values))
                kf.pr_score = si
                scored.append((si, i))
            elif kf.pr_words == min_c:
                self.branches.add("count_equal_min_unscored")
        acc_list, _ = self._accumulate(scored, q.id, "pr_query", "pr_score", {i for _, i in scored})
        order = sorted(range(len(acc_list)), key=lambda t: -float(acc_list[t][0]))     # stable, descending: list::sort(compFirst)
        loop, merge, added = [], [], set()
        for t in order:
            if not (len(loop) < n_candidates or len(merge) < n_candidates):
                break
            i = acc_list[t][1]
            kf = self.kf[i]
            if kf.bad:
                self.branches.add("bad_keyframe_skipped")
                continue
            if i in added:
                self.branches.add("duplicate_best")
                continue
            if q.map == kf.map and len(loop) < n_candidates:
                loop.append(i); self.branches.add("loop_candidate")
            elif q.map != kf.map and len(merge) < n_candidates and not self.g.map_bad[kf.map]:
                merge.append(i); self.branches.add("merge_candidate")
            elif q.map != kf.map and self.g.map_bad[kf.map] and len(merge) < n_candidates:
                self.branches.add("merge_map_bad")
            elif q.map == kf.map:
                self.branches.add("loop_full_merge_filling")
            else:
                self.branches.add("merge_full_loop_filling")
            added.add(i)
        return loop, merge

    def reloc(self, f, m):
        f_id, words, values = self.g.frames[f]
        words, values = [int(w) for w in words], [float(v) for v in values]
        sharing = []
        for w in words:
            for i in self.inverted[w]:
                kf = self.kf[i]
                if kf.rl_query != f_id:
                    kf.rl_words = 0
                    kf.rl_query = f_id
                    sharing.append(i)
                elif i not in sharing:
                    self.branches.add("stale_marker_reloc")
                kf.rl_words += 1
        if not sharing:
            self.branches.add("reloc_nothing_shared")
            return []
        max_c = max(self.kf[i].rl_words for i in sharing)
        min_c = min_common(max_c)
        scored = []
        for i in sharing:
            kf = self.kf[i]
            if kf.rl_words == min_c:
                self.branches.add("count_equal_min_unscored")
            if kf.rl_words > min_c:
                if kf.rl_words == min_c + 1:
                    self.branches.add("count_one_above_min")
                si = F32(l1_score(words, values, kf.words, kf.values))
                kf.rl_score = si
                scored.append((si, i))
        acc_list, best_acc = self._accumulate(scored, f_id, "rl_query", "rl_score", {i for _, i in scored})
        retain = F32(0.75) * best_acc
        out, added = [], set()
        for acc, i in acc_list:
            if acc > retain:
                if self.kf[i].map != m:
                    self.branches.add("reloc_other_map")
                    continue
                if i not in added:
                    out.append(i); added.add(i)
                else:
                    self.branches.add("duplicate_best")
            else:
                self.branches.add("reloc_cut_by_075")
        return out

    def state(self):
        marker = np.array([[k.pr_query, k.pr_words, k.rl_query, k.rl_words] for k in self.kf], np.int64).reshape(-1, 4)
        score = np.array([[k.pr_score, k.rl_score] for k in self.kf], np.float32).reshape(-1, 2)
        return marker, score


def run_script(g, ops):
    """Per query of the script a dict as host.kfdb_restatement returns, and the set of branches taken."""
    ref, out = Reference(g), []
    for code, a, b in np.asarray(ops).reshape(-1, 3).tolist():
        if code == sk.ADD:
            ref.add(a)
        elif code == sk.ERASE:
            ref.erase(a)
        elif code == sk.CLEAR_MAP:
            ref.clear_map(a)
        elif code == sk.CLEAR:
            ref.clear()
        else:
            loop, merge = ref.nbest(a, b) if code == sk.NBEST else (ref.reloc(a, b), [])
            marker, score = ref.state()
            out.append(dict(loop=loop, merge=merge, marker=marker, score=score))
    return out, ref.branches


def assert_same_script(got, exp, what):
    assert len(got) == len(exp), (what, len(got), len(exp))
    for q, (a, b) in enumerate(zip(got, exp)):
        assert a["loop"] == b["loop"] and a["merge"] == b["merge"], (what, q, a["loop"], b["loop"], a["merge"], b["merge"])
        assert np.array_equal(a["marker"], b["marker"]), (what, q, "markers")
        assert np.array_equal(np.asarray(a["score"], np.float32).view(np.uint32), np.asarray(b["score"], np.float32).view(np.uint32)), (what, q, "score bits")


# every branch the committed cases have to take together.  `if(lScoreAndMatch.empty()) return;` (:668, :789) cannot be taken: the
# listed keyframe with maxCommonWords words has more than (int)(maxCommonWords * 0.8f) of them, so it is always scored.
BRANCHES = {"count_equal_min_unscored", "count_one_above_min", "first_word_tie", "connected_not_listed", "connected_has_largest_count",
            "stale_marker_nbest", "stale_marker_reloc", "neighbour_listed_unscored_stale_score", "neighbour_becomes_best",
            "duplicate_best", "bad_keyframe_skipped", "loop_candidate", "merge_candidate", "merge_map_bad", "loop_full_merge_filling",
            "merge_full_loop_filling", "reloc_cut_by_075", "reloc_other_map", "nbest_nothing_shared", "reloc_nothing_shared"}

# (name, seed, keyword arguments of synth_kfdb.make_graph)
CASES = [("small_a", 11, {}), ("small_b", 12, {}), ("small_c", 13, {}), ("dense", 14, dict(n_kf=40, n_words=30, max_len=18)),
         ("sparse", 15, dict(n_kf=30, n_words=160, max_len=30)), ("two_maps", 16, dict(n_maps=2, p_bad=0.3)),
         ("long_lists", 17, dict(n_kf=60, n_words=64, max_len=40, max_cov=20))]


def build_case(name):
    seed, kw = next((s, kw) for n, s, kw in CASES if n == name)
    g = sk.make_graph(seed, **kw)
    return g, sk.make_script(seed, g, n_queries=22)


def hand_case():
    """Six words, four keyframes of map 0 and one of map 1, values that are exact in binary.  Worked by hand in
    test_kfdb_cpu.test_hand_computed_answers."""
    bow = [([0, 1, 2], [0.5, 0.25, 0.25]),        # kf 0
           ([1, 2, 3, 4], [0.25, 0.25, 0.25, 0.25]),   # kf 1
           ([0, 5], [0.5, 0.5]),                  # kf 2
           ([1, 2, 3], [0.5, 0.25, 0.25]),        # kf 3, map 1
           ([0, 1, 2, 3], [0.25, 0.25, 0.25, 0.25])]   # kf 4: the query
    g = sk.KfdbGraph(6, kf_id=[1, 2, 3, 4, 9], kf_map=[0, 0, 0, 1, 0], kf_bad=[0] * 5,
                     bow=[(np.asarray(w, np.int32), np.asarray(v, np.float64)) for w, v in bow],
                     cov=[[1], [0], [], [], []], con=[[], [], [], [], []], map_bad=[0, 0],
                     frames=[(7, np.asarray([0, 5], np.int32), np.asarray([0.75, 0.25], np.float64))])
    ops = [(sk.ADD, 0, 0), (sk.ADD, 1, 0), (sk.ADD, 2, 0), (sk.ADD, 3, 0), (sk.NBEST, 4, 2), (sk.RELOC, 0, 0)]
    return g, np.asarray(ops, np.int32)
