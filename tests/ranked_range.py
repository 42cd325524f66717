"""Expected values of the docID-range ranked tests: the unranged models (tests/ranked_or.py,
tests/ranked.py) asked for EVERY match, filtered to lo <= docID < hi, and cut to the best k by descending score, equal
scores by ascending docID. The range is a filter: a match keeps the score the unranged model gives it, bit for bit. Also
the blocks of a list that can hold a docID of a range, over numpy (what dint_query_lookup.hpp's list_blocks_in_range and the
calls' blocks_decoded are held to)."""
import numpy as np

import ranked
import ranked_or


def every_match(lists, terms, norm_lens_, num_docs: int, conjunctive: bool):
    """-> (scores f32[m], docids u32[m]) of every document the unranged call matches, best first."""
    if len(terms) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.uint32)
    k_all = max(1, sum(int(lists.postings(int(t))[0].size) for t in set(int(t) for t in terms)))  # (no fewer than the matches)
    model = ranked.ranked_and if conjunctive else ranked_or.ranked_or
    n, scores, ids = model(lists, terms, norm_lens_, num_docs, k_all)
    return scores[:n], ids[:n]


def top_in_range(matches, lo: int, hi: int, k: int):
    """every_match's pair filtered to [lo, hi) -> (count, scores f32[k], docids u32[k], matches in range), the outputs
    filled as the device fills them: 0.0 / 0xFFFFFFFF past the count."""
    sc, ids = matches
    keep = (ids.astype(np.int64) >= int(lo)) & (ids.astype(np.int64) < int(hi))
    sc, ids = sc[keep], ids[keep]
    best = np.lexsort((ids, -sc))[:k]
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    scores[:best.size] = sc[best]
    docids[:best.size] = ids[best]
    return best.size, scores, docids, int(keep.sum())


def ranked_or_range(lists, terms, norm_lens_, num_docs: int, k: int, lo: int, hi: int):
    return top_in_range(every_match(lists, terms, norm_lens_, num_docs, False), lo, hi, k)


def ranked_and_range(lists, terms, norm_lens_, num_docs: int, k: int, lo: int, hi: int):
    return top_in_range(every_match(lists, terms, norm_lens_, num_docs, True), lo, hi, k)


def merge_topk(parts, k: int):
    """The per-slice answers (count, scores, docids, ...) of ranges that tile a docID interval -> the interval's own
    (count, scores f32[k], docids u32[k])."""
    sc = np.concatenate([np.asarray(p[1])[:int(p[0])] for p in parts]) if parts else np.zeros(0, np.float32)
    ids = np.concatenate([np.asarray(p[2])[:int(p[0])] for p in parts]) if parts else np.zeros(0, np.uint32)
    return top_in_range((sc.astype(np.float32), ids.astype(np.uint32)), 0, 1 << 32, k)[:3]


def slices(lo: int, hi: int, s: int):
    """[lo, hi) cut into s consecutive half-open ranges (the last takes the remainder)."""
    cuts = [lo + (hi - lo) * i // s for i in range(s)] + [hi]
    return [(cuts[i], cuts[i + 1]) for i in range(s)]


def blocks_in_range(maxima, lo: int, hi: int):
    """The positions [p0, p1) of a list's blocks that can hold a docID of [lo, hi): maxima = the blocks' last docIDs,
    ascending. p0 = lower_bound(maxima, lo), p1 = min(nb, lower_bound(maxima, hi - 1) + 1); lo >= hi: none."""
    m = np.asarray(maxima, dtype=np.uint64)
    if lo >= hi:
        return 0, 0
    p0 = int(np.searchsorted(m, np.uint64(lo), side="left"))
    p1 = min(m.size, int(np.searchsorted(m, np.uint64(hi - 1), side="left")) + 1)
    return p0, p1


def n_blocks_in_range(blocks, term: int, lo: int, hi: int) -> int:
    """... counted for list `term` of a host block table (dint_index_posting_lists' records)."""
    p0, p1 = blocks_in_range(blocks["max"][blocks["list"] == term], lo, hi)
    return p1 - p0


BATCH_SEED = 1  # (chosen on the CPU, tests/test_ranked_range_cpu.py: with it either entry's batch matches more than 500 documents on every corpus)


def ranged_batch(queries, num_docs: int, seed: int = BATCH_SEED):
    """queries -> (queries + copies of its first 12, a range per query): widths from one docID up to past the whole docID
    space, log-uniform, anywhere in it; the copies put the same terms into several queries under different ranges; the
    first three ranges are one docID, the whole space exactly and the unrestricted range."""
    rs = np.random.RandomState(seed)
    qs = list(queries) + [list(q) for q in queries[:12]]
    ranges = []
    for i in range(len(qs)):
        width = int(round(float(np.exp(rs.uniform(0.0, np.log(2.0 * num_docs))))))
        lo = int(rs.randint(0, max(1, num_docs - min(width, num_docs) + 1)))
        ranges.append((lo, min(lo + max(1, width), 0xFFFFFFFF)))
    mid = num_docs // 2
    ranges[:3] = [(mid, mid + 1), (0, num_docs), (0, 0xFFFFFFFF)]
    return qs, np.array(ranges, dtype=np.uint32)
