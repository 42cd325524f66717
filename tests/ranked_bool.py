"""Expected values of the ranked boolean query tests: a CPU model of dint_ranked_bool_queries (include/dint_hip.h; DESIGN.md
4d-bool) in binary32, built on tests/ranked.py — required terms as ranked_and scores them, then the optional terms whose
list holds the match in ascending term id; the matches are the intersection of the required lists less every excluded list.
blocks_decoded_single is what a call of this one query claims behind the AND rounds: per excluded term (ascending id) the
blocks the candidates still alive fall in, then per required and per optional term the blocks the matches fall in — a docID
past a list's last claims nothing. A float64 form of the same sums is there for a tolerance cross-check only."""
import math

import numpy as np

import ranked
from maxscore import block_maxima, blocks_of
from queries import heavy_queries, reference_queries


def claimed_blocks(d: np.ndarray, docs: np.ndarray) -> int:
    """The distinct blocks of list d that the docIDs `docs` fall in: the first block whose last docID is >= the docID."""
    if d.size == 0 or docs.size == 0:
        return 0
    bm = block_maxima(d)
    blk = np.searchsorted(bm, docs, side="left")
    return int(np.unique(blk[blk < bm.size]).size)


def _evaluate(lists, must, should, exclude):
    """-> None for an empty `must`, else (required terms in scoring order, qf, df, their freqs at the matches; the matches;
    [(optional term, qf, df, held mask, freqs at the held matches)]; blocks_decoded_single)."""
    if len(must) == 0:
        return None
    t, qf, df, cur, fr = ranked._matches(lists, must)
    blocks = 0
    alive = np.ones(cur.size, dtype=bool)
    for x in ranked.query_freqs(exclude)[0] if len(exclude) else []:
        d = lists.postings(int(x))[0]
        blocks += claimed_blocks(d, cur[alive])
        alive &= ~np.isin(cur, d)
    cur = cur[alive]
    fr = [f[alive] for f in fr]
    for x in t:
        blocks += claimed_blocks(lists.postings(int(x))[0], cur)
    opt = []
    st, sqf = ranked.query_freqs(should) if len(should) else ((), ())
    for x, n in zip(st, sqf):
        d, f = lists.postings(int(x))
        blocks += claimed_blocks(d, cur)
        held = np.isin(cur, d)
        opt.append((int(x), int(n), int(d.size), held, f[np.searchsorted(d, cur[held])]))
    return t, qf, df, fr, cur, opt, blocks


def ranked_bool(lists, must, should, exclude, norm_lens, num_docs: int, k: int):
    """-> (count, matches, scores f32[k], docids u32[k], blocks_decoded_single): the best k matches by descending score,
    equal scores by ascending docID, 0.0 / 0xFFFFFFFF past the count."""
    scores = np.zeros(k, dtype=np.float32)
    ids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    ev = _evaluate(lists, must, should, exclude)
    if ev is None:
        return 0, 0, scores, ids, 0
    t, qf, df, fr, cur, opt, blocks = ev
    nl = np.asarray(norm_lens, dtype=np.float32)[cur]
    score = np.zeros(cur.size, dtype=np.float32)
    for j in range(t.size):
        score = score + ranked.query_term_weight(int(qf[j]), int(df[j]), num_docs) * ranked.doc_term_weight(fr[j], nl)
    for _, n, d_size, held, f in opt:
        score[held] = score[held] + ranked.query_term_weight(n, d_size, num_docs) * ranked.doc_term_weight(f, nl[held])
    best = np.lexsort((cur, -score))[:k]
    n = best.size
    scores[:n] = score[best]
    ids[:n] = cur[best]
    return n, int(cur.size), scores, ids, blocks


def ranked_bool_f64(lists, must, should, exclude, norm_lens, num_docs: int):
    """The same scores in float64 (math.log, no rounding to binary32) -> {docid: score}, for a cross-check only."""
    ev = _evaluate(lists, must, should, exclude)
    if ev is None:
        return {}
    t, qf, df, fr, cur, opt, _ = ev

    def addend(n, d_size, f, nl):
        idf = math.log((num_docs - float(d_size) + 0.5) / (float(d_size) + 0.5))
        return float(n) * max(1e-6, idf) * 2.2 * (f / (f + 1.2 * (0.5 + 0.5 * nl)))

    out = {}
    at = [np.cumsum(o[3]) - 1 for o in opt]  # a held match's place among the held ones
    for i, d in enumerate(cur.tolist()):
        nl = float(norm_lens[d])
        s = 0.0
        for j in range(t.size):
            s += addend(qf[j], df[j], float(fr[j][i]), nl)
        for (_, n, d_size, held, f), place in zip(opt, at):
            if held[i]:
                s += addend(n, d_size, float(f[place[i]]), nl)
        out[d] = s
    return out


def model_batch(lists, must, should, exclude, norm_lens, num_docs: int, k: int):
    """The model over a batch -> (counts u64[n], matches u64[n], scores f32[n, k], docids u32[n, k], [blocks_decoded_single])."""
    n = len(must)
    should = should if should is not None else [[]] * n
    exclude = exclude if exclude is not None else [[]] * n
    out = [ranked_bool(lists, must[q], should[q], exclude[q], norm_lens, num_docs, k) for q in range(n)]
    return (np.array([o[0] for o in out], dtype=np.uint64), np.array([o[1] for o in out], dtype=np.uint64),
            np.stack([o[2] for o in out]) if out else np.zeros((0, k), np.float32),
            np.stack([o[3] for o in out]) if out else np.zeros((0, k), np.uint32), [o[4] for o in out])


def split_clauses(queries, lens):
    """The GPU tests' clauses, derived from plain queries: a query of >= 3 distinct terms gives its rarest two as `must`, the
    next as `should`, and — every third such query — its most frequent as `exclude` (of three terms: the optional one
    itself, the clauses are independent); any other query is all `must`."""
    must, should, exclude = [], [], []
    n3 = 0
    for q in queries:
        u = sorted(set(int(t) for t in q), key=lambda t: (int(lens[t]), t))
        if len(u) < 3:
            must.append(list(q)), should.append([]), exclude.append([])
            continue
        n3 += 1
        must.append(u[:2])
        should.append([u[2]])
        exclude.append([u[-1]] if n3 % 3 == 0 else [])
    return must, should, exclude


def gpu_batch_clauses(lens):
    """The clauses of the GPU tests' batch over an index of these list lengths: the reference's log and 120 heavy queries."""
    return split_clauses(reference_queries(len(lens)) + heavy_queries(lens, 120), lens)


def all_blocks(lens, must, should, exclude) -> int:
    """Every block of every distinct term of every clause: what a call that is not lazy would decode."""
    return sum(blocks_of(int(lens[t])) for c in (must, should, exclude) for t in set(c))


def laziest_heavy_query(lists, lens, norm_lens, num_docs: int):
    """Of 40 heavy queries with all three clauses and a match, the one whose claims are the smallest part of its terms' blocks ->
    ((must, should, exclude), blocks claimed, all blocks)."""
    best = None
    for mu, sh, ex in zip(*split_clauses(heavy_queries(lens, 40), lens)):
        if not (sh and ex):
            continue
        claimed, every = ranked_bool(lists, mu, sh, ex, norm_lens, num_docs, 10)[4], all_blocks(lens, mu, sh, ex)
        if claimed and (best is None or claimed * best[2] < best[1] * every):
            best = ((mu, sh, ex), claimed, every)
    return best
