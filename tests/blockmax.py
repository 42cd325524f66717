"""Expected values of the block-maxima tests: a CPU model of dint_index_max_weights and of
dint_ranked_or_maxscore_queries under a wand handle with block maxima ("block maxima"), built from
the pruned model (tests/maxscore.py) and its BM25 pieces (tests/ranked.py).

block_max_weights: per block of the index (lists in order, each cut as maxscore.blocks_of cuts it) the largest
doc_term_weight of its postings, the maximum starting at 0.0f and taking a value only if it is larger (a NaN never enters).

maxscore_blockmax: steps 1-6 of maxscore.maxscore with one change in step 4. The seed, theta, the split into N and E by
TERM maxima, the claims, the scores and the selection are that model's. A candidate d dies not only if
(P + sum_N m_t) * margin < theta but also if (P + R(d)) * margin < theta with R(d), from 0.0 in double over the N terms in
ascending term id, the sum of (double) fl32(q_w_t * block_max_weight[b_t(d)]), b_t(d) the first block of t whose last docID
is >= d; a term whose list ends before d adds nothing. A seed that sits in N is bounded like any other N term. (Block
maxima no larger than their list's term maximum make R(d) the smaller sum: the rule is then (P + R(d)) * margin < theta
alone. Taking the smaller of the two is what makes larger block maxima, up to +inf, harmless: the blocks read never
exceed the term-maxima call's, and under +inf they equal them — only candidates beyond every N list can still die, and
those claim nothing.)"""
import numpy as np

import maxscore
import ranked
import ranked_or
from maxscore import BLOCK, Result, block_maxima, blocks_of


def block_firsts(bounds) -> np.ndarray:
    """Per list, its first block in the index's block table (n_lists + 1 entries: the last is the block count)."""
    lens = np.diff(np.asarray(bounds).astype(np.int64))
    return np.concatenate([[0], np.cumsum((lens + BLOCK - 1) // BLOCK)]).astype(np.int64)


def block_max_weights(docids, freqs, bounds, nl) -> np.ndarray:
    """dint_index_max_weights' block_max_weight: one float per block, in block-table order."""
    first = block_firsts(bounds)
    out = np.zeros(int(first[-1]), dtype=np.float32)
    nl = np.asarray(nl, dtype=np.float32)
    for t in range(len(bounds) - 1):
        lo, hi = int(bounds[t]), int(bounds[t + 1])
        if hi == lo:
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            w = ranked.doc_term_weight(freqs[lo:hi], nl[docids[lo:hi]])
        w = np.where(w > 0, w, np.float32(0)).astype(np.float32)  # (what std::max(max, score) from 0.0f lets in)
        out[first[t]:first[t + 1]] = np.maximum.reduceat(w, np.arange(0, hi - lo, BLOCK))
    return out


def term_maxima_of_blocks(bmw: np.ndarray, bounds) -> np.ndarray:
    """dint_index_max_weights' max_term_weight: the largest block maximum of every list, 0.0f for a list without a block."""
    first = block_firsts(bounds)
    out = np.zeros(len(bounds) - 1, dtype=np.float32)
    for t in range(out.size):
        if first[t + 1] > first[t]:
            out[t] = bmw[first[t]:first[t + 1]].max()
    return out


def maxscore_blockmax(lists, terms, norm_lens_, max_term_weight, block_max_weight, num_docs: int, k: int) -> Result:
    scores = np.zeros(k, dtype=np.float32)
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    if len(terms) == 0:
        return Result(0, scores, ids)
    norm_lens_ = np.asarray(norm_lens_, dtype=np.float32)
    first = block_firsts(lists.bounds)
    t, qf, post, union = ranked_or._union(lists, terms)
    df = np.array([p[0].size for p in post], dtype=np.int64)
    nb = np.array([blocks_of(int(x)) for x in df], dtype=np.int64)
    union_scores = maxscore._scores(t, qf, post, union, norm_lens_[union], num_docs)
    if union.size == 0:
        return Result(0, scores, ids)
    n = t.size
    qw = [ranked.query_term_weight(int(qf[j]), int(df[j]), num_docs) for j in range(n)]
    addend = lambda j: qw[j] * ranked.doc_term_weight(post[j][1], norm_lens_[post[j][0]])
    plan = np.lexsort((t, -df))
    # 1. the seed and theta
    seeds = [j for j in range(n) if df[j] >= k]
    seed = min(seeds, key=lambda j: (int(df[j]), int(t[j]))) if seeds else None
    theta = np.float32(0)
    if seed is not None:
        theta = np.sort(addend(seed))[::-1][k - 1]
    # 2. the split, by term maxima
    margin = 1.0 + (n + 1) * 2.0 ** -23
    with np.errstate(over="ignore"):
        m = [np.float32(qw[j] * np.float32(max_term_weight[int(t[j])])) for j in range(n)]
    in_n = np.zeros(n, dtype=bool)
    rest = 0.0
    if theta > 0:
        for j in sorted(range(n), key=lambda j: (m[j], int(t[j])))[:n - 1]:
            nxt = rest + float(m[j])
            if not nxt * margin < float(theta):
                break
            rest = nxt
            in_n[j] = True
    e_plan = [int(j) for j in plan if not in_n[j]]
    # 3. the candidates
    cand = np.zeros(0, dtype=np.uint32)
    for j in e_plan:
        cand = np.union1d(cand, post[j][0]).astype(np.uint32)
    P = np.zeros(cand.size, dtype=np.float64)
    for j in e_plan:
        d = post[j][0]
        if d.size == 0:
            continue
        pos = np.minimum(np.searchsorted(d, cand), d.size - 1)
        hit = d[pos] == cand
        P[hit] = P[hit] + addend(j)[pos[hit]].astype(np.float64)
    # 4. the bound, by block maxima: per candidate, over N in ascending term id (t is ascending)
    R = np.zeros(cand.size, dtype=np.float64)
    for j in range(n):
        if not in_n[j] or df[j] == 0:
            continue
        pos = np.searchsorted(block_maxima(post[j][0]), cand, side="left")
        inside = pos < nb[j]
        bm = np.asarray(block_max_weight, dtype=np.float32)[first[int(t[j])] + pos[inside]]
        with np.errstate(over="ignore", invalid="ignore"):
            R[inside] = R[inside] + (qw[j] * bm).astype(np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        live = cand[~((P + np.minimum(R, rest)) * margin < float(theta))]
    # 5. the claims
    read = sum(int(nb[j]) for j in range(n) if not in_n[j] or j == seed)
    for j in range(n):
        if in_n[j] and j != seed and df[j]:
            pos = np.searchsorted(block_maxima(post[j][0]), live, side="left")
            read += int(np.unique(pos[pos < nb[j]]).size)
    # 6. score and select
    sc = union_scores[np.searchsorted(union, live)]
    best = np.lexsort((live, -sc))[:k]
    c = best.size
    scores[:c] = sc[best]
    ids[:c] = live[best]
    return Result(c, scores, ids, read, float(theta), live, union, union_scores, len(e_plan), int(nb.sum()))


# ---------------------------------------------------------------------------------------------------------------
# the hand-made case where the gain is certain
# ---------------------------------------------------------------------------------------------------------------
GAIN_NUM_DOCS = 100_000
GAIN_K = 10
GAIN_BLOCK = 11  # the block of the long list that holds its one high-freq posting


def certain_gain():
    """-> (lists, freqs, num_docs, norm_lens, query). Every norm_len is 1. List 0 (the seed): 600 postings, docIDs
    150 i + 7, freq 2 but for ten of freq 50 (i = 250 .. 259); list 1: 7168 postings (28 blocks), docIDs 13 i, freq 1 but
    for ONE posting of freq 1000 in block 11 (docIDs 36608 .. 39923, where the seed's ten best and thirteen more of its
    documents fall). theta is the seed's addend at freq 50; list 1's term maximum (freq 1000) is below it, so list 1 is in
    N; a seed document of freq 2 plus that term maximum reaches theta — the term bound keeps all 600 candidates and
    they claim every block of list 1 — but plus the block maximum of a freq-1 block it does not: the block bound keeps
    the 23 candidates of block 11 only. Blocks read: 3 + 28 against 3 + 1."""
    seed = (150 * np.arange(600) + 7).astype(np.uint32)
    seed_f = np.full(600, 2, dtype=np.uint32)
    seed_f[250:260] = 50
    long_ = (13 * np.arange(7168)).astype(np.uint32)
    long_f = np.ones(7168, dtype=np.uint32)
    long_f[BLOCK * GAIN_BLOCK + 100] = 1000
    return [seed, long_], [seed_f, long_f], GAIN_NUM_DOCS, np.ones(GAIN_NUM_DOCS, dtype=np.float32), [0, 1]
