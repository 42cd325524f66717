"""Expected values of the union-driven ranked boolean query tests: a CPU model of dint_ranked_or_bool_queries
(include/dint_hip.h) in binary32, built on tests/ranked_or.py — the union of the optional lists with,
per document, the number of distinct lists that hold it; the documents in fewer than m = max(1, min_should_match) lists
dropped; then the excluded terms in ascending term id, each claiming (ranked_bool.claimed_blocks) the blocks of its list the
documents still alive fall in before it removes the ones it holds; ranked_or's scores for the survivors; lexsort.
blocks_decoded_single is what a call of this one query reports: every block of its distinct optional terms plus those
claims — 0 for a query that cannot match (no block in its lists, or m above its distinct terms). A float64 form of the same
sums is there for a tolerance cross-check only."""
import numpy as np

import ranked
import ranked_or
from maxscore import blocks_of
from queries import heavy_queries, reference_queries
from ranked_bool import claimed_blocks


class Evaluated:
    """One query, before the top k is cut: its matches ascending, their binary32 scores, and the blocks a call of it decodes
    (eager: the optional terms'; lazy: per excluded term in ascending id, (term, claimed, blocks of its list))."""

    def __init__(self, docs, scores, eager, lazy):
        self.docs, self.scores, self.eager, self.lazy = docs, scores, eager, lazy

    @property
    def blocks(self) -> int:
        return self.eager + sum(c for _, c, _ in self.lazy)

    def top(self, k: int):
        """-> (count, matches, scores f32[k], docids u32[k], blocks_decoded_single): the best k by descending score, equal
        scores by ascending docID, 0.0 / 0xFFFFFFFF past the count."""
        scores = np.zeros(k, dtype=np.float32)
        ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
        best = np.lexsort((self.docs, -self.scores))[:k]
        n = best.size
        scores[:n] = self.scores[best]
        ids[:n] = self.docs[best]
        return n, int(self.docs.size), scores, ids, self.blocks


_NOTHING = Evaluated(np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, [])


def distinct(terms):
    return sorted(set(int(t) for t in terms))


def evaluate(lists, should, exclude, m, norm_lens, num_docs: int) -> Evaluated:
    m = max(1, int(m) if m is not None else 1)
    if len(should) == 0:
        return _NOTHING
    t, qf, post, cur = ranked_or._union(lists, should)
    eager = sum(blocks_of(int(d.size)) for d, _ in post)
    if eager == 0 or m > t.size:
        return _NOTHING
    nl = np.asarray(norm_lens, dtype=np.float32)[cur]
    score = np.zeros(cur.size, dtype=np.float32)
    held = np.zeros(cur.size, dtype=np.int64)
    for j in range(t.size):  # ascending term id: ranked_or.ranked_or's sum
        d, f = post[j]
        if d.size == 0:
            continue
        pos = np.minimum(np.searchsorted(d, cur), d.size - 1)
        hit = d[pos] == cur
        score[hit] = score[hit] + ranked.query_term_weight(int(qf[j]), int(d.size), num_docs) * ranked.doc_term_weight(f[pos][hit], nl[hit])
        held += hit
    alive = held >= m
    lazy = []
    for x in distinct(exclude if exclude is not None else []):
        d = lists.postings(x)[0]
        lazy.append((x, claimed_blocks(d, cur[alive]), blocks_of(int(d.size))))
        alive &= ~np.isin(cur, d)
    return Evaluated(cur[alive], score[alive], eager, lazy)


def ranked_or_bool(lists, should, exclude, m, norm_lens, num_docs: int, k: int):
    """-> (count, matches, scores f32[k], docids u32[k], blocks_decoded_single)."""
    return evaluate(lists, should, exclude, m, norm_lens, num_docs).top(k)


def ranked_or_bool_f64(lists, should, exclude, m, norm_lens, num_docs: int):
    """The matches' scores in float64 (ranked_or.ranked_or_f64: math.log, no rounding to binary32) -> {docid: score}, from
    plain set arithmetic: for a cross-check only."""
    u = distinct(should)
    m = max(1, int(m) if m is not None else 1)
    if not u or m > len(u):
        return {}
    held = {}
    for t in u:
        for d in lists.postings(t)[0].tolist():
            held[d] = held.get(d, 0) + 1
    gone = set()
    for t in distinct(exclude if exclude is not None else []):
        gone.update(lists.postings(t)[0].tolist())
    f64 = ranked_or.ranked_or_f64(lists, should, norm_lens, num_docs)
    return {d: f64[d] for d, n in held.items() if n >= m and d not in gone}


def evaluate_batch(lists, should, exclude, mins, norm_lens, num_docs: int):
    n = len(should)
    exclude = exclude if exclude is not None else [[]] * n
    mins = mins if mins is not None else [1] * n
    return [evaluate(lists, should[q], exclude[q], mins[q], norm_lens, num_docs) for q in range(n)]


def top_batch(evs, k: int):
    """The model over a batch -> (counts u64[n], matches u64[n], scores f32[n, k], docids u32[n, k], [blocks_decoded_single])."""
    out = [e.top(k) for e in evs]
    return (np.array([o[0] for o in out], dtype=np.uint64), np.array([o[1] for o in out], dtype=np.uint64),
            np.stack([o[2] for o in out]) if out else np.zeros((0, k), np.float32),
            np.stack([o[3] for o in out]) if out else np.zeros((0, k), np.uint32), [o[4] for o in out])


def model_batch(lists, should, exclude, mins, norm_lens, num_docs: int, k: int):
    return top_batch(evaluate_batch(lists, should, exclude, mins, norm_lens, num_docs), k)


def derive_clauses(queries, lens):
    """The GPU tests' clauses, derived from plain queries -> (should, exclude, min_should_match). u: the query's distinct
    terms, rarest first. The i-th query of >= 2 distinct terms is, by i % 4: 0 the query itself (repeats kept) with m = 2;
    1 the query less its most frequent term, that term excluded, m = 1; 2 the same with m = 2 where two terms are left;
    3 the query itself, m = 0 (as 1). The i-th query of one distinct term is, by i % 3: 0 its term optional and excluded (the
    clauses are independent: nothing is left); 1 m = 2 (above its terms: nothing); 2 itself."""
    should, exclude, mins = [], [], []
    n2 = n1 = 0
    for q in queries:
        q = [int(t) for t in q]
        u = sorted(set(q), key=lambda t: (int(lens[t]), t))
        if len(u) >= 2:
            kind, n2 = n2 % 4, n2 + 1
            rest = [t for t in q if t != u[-1]]
            should.append(q if kind in (0, 3) else rest)
            exclude.append([u[-1]] if kind in (1, 2) else [])
            mins.append((2, 1, 2 if len(u) >= 3 else 1, 0)[kind])
        else:
            kind, n1 = n1 % 3, n1 + 1
            should.append(q)
            exclude.append(list(q) if kind == 0 else [])
            mins.append(2 if kind == 1 else 1)
    return should, exclude, mins


def gpu_batch_clauses(lens):
    """The clauses of the GPU tests' batch over an index of these list lengths: the reference's log and 120 heavy queries."""
    return derive_clauses(reference_queries(len(lens)) + heavy_queries(lens, 120), lens)
