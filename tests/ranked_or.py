"""Expected values of the ranked-OR tests: a CPU model of ranked_or_query (include/ds2i/queries.hpp:387-457) in binary32,
built from the ranked-AND model's BM25 pieces (tests/ranked.py). Every document of the union of a query's lists scores
0.0f plus, for each distinct term in ascending term id (the order query_freqs returns), q_weight * doc_term_weight for
the terms whose list holds it. A plain Python float64 form of the same sums is there only as a cross-check."""
import math

import numpy as np

import ranked


def _union(lists, terms):
    """-> (distinct terms ascending, their qf, per term its (docids, freqs), the union's docIDs ascending)."""
    t, qf = ranked.query_freqs(terms)
    post = [lists.postings(int(x)) for x in t]
    cur = np.zeros(0, dtype=np.uint32)
    for d, _ in post:
        cur = np.union1d(cur, d).astype(np.uint32)
    return t, qf, post, cur


def ranked_or(lists, terms, norm_lens_, num_docs: int, k: int):
    """ranked_or_query with the top-k as the device returns it -> (count, scores f32[k], docids u32[k]): the best k by
    descending score, equal scores by ascending docID, 0.0 / 0xFFFFFFFF past the count."""
    scores = np.zeros(k, dtype=np.float32)
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    if len(terms) == 0:
        return 0, scores, ids
    t, qf, post, cur = _union(lists, terms)
    nl = np.asarray(norm_lens_, dtype=np.float32)[cur]
    score = np.zeros(cur.size, dtype=np.float32)
    for j in range(t.size):  # ascending term id
        d, f = post[j]
        if d.size == 0:
            continue
        pos = np.minimum(np.searchsorted(d, cur), d.size - 1)
        hit = d[pos] == cur
        w = ranked.query_term_weight(int(qf[j]), int(d.size), num_docs) * ranked.doc_term_weight(f[pos][hit], nl[hit])
        score[hit] = score[hit] + w
    best = np.lexsort((cur, -score))[:k]
    n = best.size
    scores[:n] = score[best]
    ids[:n] = cur[best]
    return n, scores, ids


def ranked_or_f64(lists, terms, norm_lens_, num_docs: int):
    """The same scores in float64 (math.log, no rounding to binary32) -> {docid: score}, for a cross-check only."""
    if len(terms) == 0:
        return {}
    t, qf, post, _ = _union(lists, terms)
    out = {}
    for j in range(t.size):
        d, f = post[j]
        df = float(d.size)
        idf = math.log((num_docs - df + 0.5) / (df + 0.5))
        qw = float(qf[j]) * max(1e-6, idf) * 2.2
        for doc, fr in zip(d.tolist(), f.tolist()):
            nl = float(norm_lens_[doc])
            out[doc] = out.get(doc, 0.0) + qw * (fr / (fr + 1.2 * (0.5 + 0.5 * nl)))
    return out
