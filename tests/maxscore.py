"""Expected values of the pruned ranked-OR tests: a CPU model of dint_ranked_or_maxscore_queries over
the builder's lists, built from the ranked-OR model (tests/ranked_or.py) and its BM25 pieces (tests/ranked.py).

Per query, over its distinct terms T: the seed (the shortest list of at least k postings, the smaller term id on ties)
gives theta, the k-th largest of its addends a_s(d) = fl32(q_w * doc_term_weight); N is the longest proper prefix of T by
(m_t = fl32(q_w * max_term_weight_t) ascending, term id) with (sum_N m_t, double) * margin < theta, margin = 1 + (|T| + 1)
* 2^-23, and E the rest. The candidates are the union of E's lists; one whose E addends P (double, summed in E's order:
longest list first) satisfy (P + sum_N m_t) * margin < theta is pruned; every other one claims, in each N term but the
seed, the block its docID falls in (the first block whose last docID is >= it). The survivors get ranked_or's binary32
score and the best k are kept. blocks_read = the seed's blocks + the other E terms' blocks + the claimed blocks."""
from dataclasses import dataclass, field

import numpy as np

import ranked
import ranked_or

BLOCK = 256  # postings per block of the index (dict_posting_list)


@dataclass
class Result:
    count: int
    scores: np.ndarray
    ids: np.ndarray
    blocks_read: int = 0
    theta: float = 0.0
    candidates: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))  # the survivors of the bound
    union: np.ndarray = field(default_factory=lambda: np.zeros(0, np.uint32))       # every document of the query's union
    union_scores: np.ndarray = field(default_factory=lambda: np.zeros(0, np.float32))  # their ranked_or scores
    n_essential: int = 0
    all_blocks: int = 0  # every block of every distinct term (what ranked_or reads)


def blocks_of(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


def block_maxima(d: np.ndarray) -> np.ndarray:
    """The last docID of every block of a list."""
    nb = blocks_of(d.size)
    return d[np.minimum(np.arange(nb) * BLOCK + BLOCK - 1, d.size - 1)]


def _scores(t, qf, post, cur, nl, num_docs):
    """ranked_or's binary32 scores of the documents `cur` (ascending term id, from 0.0f)."""
    score = np.zeros(cur.size, dtype=np.float32)
    for j in range(t.size):
        d, f = post[j]
        if d.size == 0:
            continue
        pos = np.minimum(np.searchsorted(d, cur), d.size - 1)
        hit = d[pos] == cur
        w = ranked.query_term_weight(int(qf[j]), int(d.size), num_docs) * ranked.doc_term_weight(f[pos][hit], nl[hit])
        score[hit] = score[hit] + w
    return score


def maxscore(lists, terms, norm_lens_, max_term_weight, num_docs: int, k: int) -> Result:
    scores = np.zeros(k, dtype=np.float32)
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    if len(terms) == 0:
        return Result(0, scores, ids)
    norm_lens_ = np.asarray(norm_lens_, dtype=np.float32)
    t, qf, post, union = ranked_or._union(lists, terms)
    df = np.array([p[0].size for p in post], dtype=np.int64)
    nb = np.array([blocks_of(int(x)) for x in df], dtype=np.int64)
    union_scores = _scores(t, qf, post, union, norm_lens_[union], num_docs)
    if union.size == 0:
        return Result(0, scores, ids)
    n = t.size
    qw = [ranked.query_term_weight(int(qf[j]), int(df[j]), num_docs) for j in range(n)]
    addend = lambda j: qw[j] * ranked.doc_term_weight(post[j][1], norm_lens_[post[j][0]])  # a_t(d) over list j
    plan = np.lexsort((t, -df))  # longest list first, equal lengths by term id
    # 1. the seed and theta
    seeds = [j for j in range(n) if df[j] >= k]
    seed = min(seeds, key=lambda j: (int(df[j]), int(t[j]))) if seeds else None
    theta = np.float32(0)
    if seed is not None:
        theta = np.sort(addend(seed))[::-1][k - 1]
    # 2. the split
    margin = 1.0 + (n + 1) * 2.0 ** -23
    with np.errstate(over="ignore"):  # (maxima up to FLT_MAX and +inf are legal upper bounds: m_t = +inf keeps t in E)
        m = [np.float32(qw[j] * np.float32(max_term_weight[int(t[j])])) for j in range(n)]
    in_n = np.zeros(n, dtype=bool)
    rest = 0.0
    if theta > 0:
        for j in sorted(range(n), key=lambda j: (m[j], int(t[j])))[:n - 1]:  # (E is never empty)
            nxt = rest + float(m[j])
            if not nxt * margin < float(theta):
                break
            rest = nxt
            in_n[j] = True
    e_plan = [int(j) for j in plan if not in_n[j]]
    # 3. the candidates and 4. their bound
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
    live = cand[~((P + rest) * margin < float(theta))]
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


def assert_degraded(count, scores, ids, res: Result, want_count: int):
    """What maxima below the true ones may do to an answer (include/dint_hip.h) and nothing else: `count` (docID, score) pairs,
    each a document of the query's union with its exact ranked_or score (res.union / res.union_scores: any model run of the
    query has them), strictly ordered by (score descending, docID ascending), no more of them than ranked_or returns."""
    count = int(count)
    assert count <= want_count <= scores.size
    got_ids, got_scores = ids[:count], scores[:count]
    pos = np.searchsorted(res.union, got_ids)
    assert (pos < res.union.size).all() and np.array_equal(res.union[np.minimum(pos, max(res.union.size - 1, 0))], got_ids)
    assert np.array_equal(res.union_scores[pos].view(np.uint32), got_scores.view(np.uint32))
    later = (got_scores[1:] < got_scores[:-1]) | ((got_scores[1:] == got_scores[:-1]) & (got_ids[1:] > got_ids[:-1]))
    assert later.all()
    assert (scores[count:] == 0).all() and (ids[count:] == 0xFFFFFFFF).all()


def mixed_queries(lens: np.ndarray, n_queries: int, seed: int = 9, pool: int = 48, lo: int = 16, hi: int = 4096):
    """One term from the rare tail (a list of lo .. hi postings outside the `pool` longest; a corpus with no such list: the
    shortest quarter of its lists) and 1-3 of the `pool` longest lists: the shape where the rare term's threshold leaves
    the long lists' blocks mostly unread."""
    r = np.random.default_rng(seed)
    order = np.argsort(-lens.astype(np.int64), kind="stable")
    big = order[:pool]
    tail = np.array([x for x in order[pool:] if lo <= lens[x] <= hi], dtype=np.int64)
    if tail.size == 0:
        nonempty = order[lens[order] > 0][::-1]
        tail = nonempty[:max(1, nonempty.size // 4)]
    out = []
    for _ in range(n_queries):
        q = [int(r.choice(tail))] + r.choice(big, min(big.size, int(r.integers(1, 4))), replace=False).tolist()
        out.append(np.array(q, dtype=np.uint32))
    return out
