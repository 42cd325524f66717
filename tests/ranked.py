"""Expected values of the ranked-query tests: a CPU model of ranked_and_query (include/ds2i/queries.hpp:309-385) and of
wand_data (include/ds2i/wand_data.hpp:18-57) in binary32, operation for operation in the reference's source order.

q_weight takes its logarithm from the C library's logf through ctypes — the function std::log(float) calls; every other
operation is a numpy float32 scalar or array operation (numpy never contracts a multiply and an add into one FMA). A plain
Python float64 form of the same sums is there only as a cross-check with a relative tolerance."""
import ctypes as C
import ctypes.util
import math

import numpy as np

F = np.float32
B, K1 = F(0.5), F(1.2)  # bm25::b, bm25::k1 (bm25.hpp)
EPSILON_SCORE = F(1.0e-6)

_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def logf(x) -> np.float32:
    return F(_libm.logf(float(F(x))))


def query_term_weight(qf: int, df: int, num_docs: int) -> np.float32:
    """bm25::query_term_weight: f * max(1e-6, idf) * (1 + k1), idf = log((N - df + 0.5) / (df + 0.5))."""
    f, fdf = F(qf), F(df)
    idf = logf((F(num_docs) - fdf + F(0.5)) / (fdf + F(0.5)))
    return f * (idf if EPSILON_SCORE < idf else EPSILON_SCORE) * (F(1.0) + K1)


def doc_term_weight(freqs, norm_lens) -> np.ndarray:
    """bm25::doc_term_weight over arrays: f / (f + k1 * ((1 - b) + b * norm_len))."""
    f = np.asarray(freqs).astype(np.float32)
    nl = np.asarray(norm_lens, dtype=np.float32)
    return f / (f + K1 * ((F(1.0) - B) + B * nl))


def norm_lens(sizes) -> np.ndarray:
    """wand_data's norm_lens: float(len) / avg_len, avg_len = float(sum of the float lens as a double / double(num_docs))."""
    lens = np.asarray(sizes).astype(np.float32)
    total = float(np.sum(lens.astype(np.float64)))  # (integers below 2^53: exact, in any order)
    avg_len = F(total / float(lens.size))
    return lens / avg_len


def max_term_weights(docids, freqs, bounds, nl) -> np.ndarray:
    """wand_data's max_term_weight: per list, the largest doc_term_weight of its postings (0 for an empty list)."""
    out = np.zeros(len(bounds) - 1, dtype=np.float32)
    for t in range(len(bounds) - 1):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        if hi > lo:
            out[t] = doc_term_weight(freqs[lo:hi], nl[docids[lo:hi]]).max()
    return out


def query_freqs(terms):
    """query_freqs (queries.hpp:135-148): distinct terms, ascending, with their multiplicity."""
    t, qf = np.unique(np.asarray(terms, dtype=np.int64), return_counts=True)
    return t, qf


class BuilderLists:
    """Lists as the index builder got them: docids / freqs back to back, list t = [bounds[t], bounds[t + 1])."""

    def __init__(self, docids, freqs, bounds):
        self.docids, self.freqs, self.bounds = docids, freqs, bounds

    def postings(self, t: int):
        lo, hi = int(self.bounds[t]), int(self.bounds[t + 1])
        return self.docids[lo:hi], self.freqs[lo:hi]


def _matches(lists, terms):
    """-> (distinct terms in scoring order, their qf, their df, the intersection's docIDs, per term the freqs at them)."""
    t, qf = query_freqs(terms)
    post = [lists.postings(int(x)) for x in t]
    df = np.array([p[0].size for p in post], dtype=np.int64)
    order = np.lexsort((t, df))  # increasing list length, equal lengths by term id
    cur = post[order[0]][0] if t.size else np.zeros(0, np.uint32)
    for j in order[1:]:
        cur = np.intersect1d(cur, post[j][0], assume_unique=True)
    fr = []
    for j in order:
        d, f = post[j]
        fr.append(f[np.searchsorted(d, cur)])
    return t[order], qf[order], df[order], cur, fr


def ranked_and(lists, terms, norm_lens_, num_docs: int, k: int):
    """ranked_and_query with the top-k as the device returns it -> (count, scores f32[k], docids u32[k]): the best k by
    descending score, equal scores by ascending docID, 0.0 / 0xFFFFFFFF past the count."""
    scores = np.zeros(k, dtype=np.float32)
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    if len(terms) == 0:
        return 0, scores, ids
    t, qf, df, cur, fr = _matches(lists, terms)
    nl = np.asarray(norm_lens_, dtype=np.float32)[cur]
    score = np.zeros(cur.size, dtype=np.float32)
    for j in range(t.size):
        score = score + query_term_weight(int(qf[j]), int(df[j]), num_docs) * doc_term_weight(fr[j], nl)
    best = np.lexsort((cur, -score))[:k]
    n = best.size
    scores[:n] = score[best]
    ids[:n] = cur[best]
    return n, scores, ids


def ranked_and_f64(lists, terms, norm_lens_, num_docs: int):
    """The same scores in float64 (math.log, no rounding to binary32) -> {docid: score}, for a cross-check only."""
    if len(terms) == 0:
        return {}
    t, qf, df, cur, fr = _matches(lists, terms)
    out = {}
    for i, d in enumerate(cur.tolist()):
        nl = float(norm_lens_[d])
        s = 0.0
        for j in range(t.size):
            idf = math.log((num_docs - float(df[j]) + 0.5) / (float(df[j]) + 0.5))
            qw = float(qf[j]) * max(1e-6, idf) * 2.2
            f = float(fr[j][i])
            s += qw * (f / (f + 1.2 * (0.5 + 0.5 * nl)))
        out[d] = s
    return out
