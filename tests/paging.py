"""Expected values of the paged ranked tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py), in the device's key order
— a higher score first, equal scores by ascending docID. A match (s, d) lies AFTER the cursor (cs, cd) iff s < cs, or s == cs
and d > cd; a page is the first k of the matches after the cursor, and skipped counts the others. page_after says this with
numpy's float comparisons; page_after_by_loop, a document at a time, builds the 64-bit keys from the floats' bits and compares
integers, as the device does (tests/test_paging_cpu.py holds the first to it). The collapsed forms cut the kept documents of
tests/collapse.py in the same way. Also the cursor draw of the fuzz cases, so that tests/test_paging_cpu.py can replay them
without a device."""
import math
import struct

import numpy as np

import collapse as CO
import doc_filter as DF

FROM_START = 0xFFFFFFFFFFFFFFFF  # the cursor key of a query that is read from the start
DRAW_SEED = 0x5AF7               # the fuzz's cursor generator: np.random.default_rng([case seed, DRAW_SEED])
DRAW_WEIGHTS = (0.7, 0.1, 0.1, 0.1)  # a match | a match's score, a random docID | from the start | a random score and docID


def in_filter(matches, mask):
    """every_match's pair under the mask (None: no filter), in key order"""
    sc, ids = matches
    if mask is not None:
        keep = DF.holds(mask, ids)
        sc, ids = sc[keep], ids[keep]
    order = np.lexsort((ids, -sc))
    return sc[order], ids[order]


def _cursor(cursor):
    """None | (score, docid) -> (the score as the binary32 the device gets, docid); None: (+inf, 0)"""
    if cursor is None:
        return np.float32(np.inf), 0
    cs = np.float32(cursor[0])
    assert not np.isnan(cs), "a NaN cursor is refused"
    return cs, int(cursor[1])


def after_cursor(sc, ids, cursor):
    """-> bool[m]: which of the documents (sc, ids) lie after the cursor. +inf: every one (every score is finite); a score
    <= 0: none."""
    cs, cd = _cursor(cursor)
    if cs <= 0:  # (the contract's rule, not the comparison's: a match whose score underflowed to 0.0 is not after a 0.0 cursor)
        return np.zeros(ids.size, dtype=bool)
    return (sc < cs) | ((sc == cs) & (ids.astype(np.int64) > cd))


def _filled(sc, ids, k):
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    scores[:sc.size] = sc
    docids[:ids.size] = ids
    return scores, docids


def page_after(matches, mask, cursor, k: int):
    """every_match's pair, the filter's mask (None: no filter) and the cursor (None: from the start) -> (count, scores f32[k],
    docids u32[k], matches, skipped), the outputs filled as the device fills them: 0.0 / 0xFFFFFFFF past the count."""
    sc, ids = in_filter(matches, mask)
    after = after_cursor(sc, ids, cursor)
    scores, docids = _filled(sc[after][:k], ids[after][:k], k)
    return min(int(after.sum()), k), scores, docids, int(ids.size), int(ids.size - after.sum())


def bits_of(score) -> int:
    return struct.unpack("<I", struct.pack("<f", float(score)))[0]


def key_of(score, docid) -> int:
    """the selection's key of a document: the score's bits, then the inverted docID"""
    return (bits_of(score) << 32) | (0xFFFFFFFF - int(docid))


def cursor_key(cursor) -> int:
    """the key the host maps a cursor to: from the start (None, +inf): FROM_START; a score <= 0, -0.0 and -inf with it: 0"""
    if cursor is None:
        return FROM_START
    cs = float(np.float32(cursor[0]))
    assert not math.isnan(cs), "a NaN cursor is refused"
    if cs == math.inf:
        return FROM_START
    return 0 if cs <= 0.0 else key_of(cs, cursor[1])


def page_after_by_loop(matches, mask, cursor, k: int):
    """page_after, a document at a time, on the keys' bits: a document is after the cursor iff its key is strictly below the
    cursor's; the page is the k largest keys of those, unpacked."""
    ck = cursor_key(cursor)
    n, keys = 0, []
    for s, d in zip(matches[0], (int(x) for x in matches[1])):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        n += 1
        key = key_of(s, d)
        if key < ck:
            keys.append(key)
    page = sorted(keys, reverse=True)[:k]
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    for i, key in enumerate(page):
        scores[i] = struct.unpack("<f", struct.pack("<I", key >> 32))[0]
        docids[i] = 0xFFFFFFFF - (key & 0xFFFFFFFF)
    return len(page), scores, docids, n, n - len(keys)


def collapsed_page_after(matches, mask, group_of, n_groups: int, cursor, k: int):
    """tests/collapse.py's collapse behind a cursor: the cursor cuts the KEPT documents, after the best of every group is
    taken -> (count, scores, docids, matches, collapsed, hit_groups, hit_group_matches, row, skipped), skipped the kept
    documents that are not after the cursor; matches, collapsed and the row are collapse's own."""
    k_all = max(1, int(matches[1].size))
    n, sc, ids, n_matches, collapsed, groups, group_matches, row = CO.collapse(matches, mask, group_of, n_groups, k_all)
    sc, ids, groups, group_matches = sc[:n], ids[:n], groups[:n], group_matches[:n]
    after = after_cursor(sc, ids, cursor)
    scores, docids = _filled(sc[after][:k], ids[after][:k], k)
    hit_groups = np.full(k, CO.DEVICE_NONE, dtype=np.uint32)
    hit_group_matches = np.zeros(k, dtype=np.uint32)
    count = min(int(after.sum()), k)
    hit_groups[:count] = groups[after][:k]
    hit_group_matches[:count] = group_matches[after][:k]
    return count, scores, docids, n_matches, collapsed, hit_groups, hit_group_matches, row, int(n - after.sum())


def collapsed_page_after_by_loop(matches, mask, group_of, n_groups: int, cursor, k: int):
    """collapsed_page_after on the keys' bits, over tests/collapse.py's per-document loop"""
    k_all = max(1, int(matches[1].size))
    n, sc, ids, n_matches, collapsed, groups, group_matches, row = CO.collapse_by_loop(matches, mask, group_of, n_groups, k_all)
    ck = cursor_key(cursor)
    at = [i for i in range(n) if key_of(sc[i], ids[i]) < ck]
    page = at[:k]
    scores, docids = _filled(sc[page], ids[page], k)
    hit_groups = np.full(k, CO.DEVICE_NONE, dtype=np.uint32)
    hit_group_matches = np.zeros(k, dtype=np.uint32)
    hit_groups[:len(page)] = groups[page]
    hit_group_matches[:len(page)] = group_matches[page]
    return len(page), scores, docids, n_matches, collapsed, hit_groups, hit_group_matches, row, n - len(at)


def stacked(per_query, k: int):
    """page_after's tuples of a batch -> the arrays as the binding returns them: (counts u64[n], scores f32[n, k], docids
    u32[n, k], matches u64[n], skipped u64[n])"""
    def rows_of(j, dtype):
        return np.stack([o[j] for o in per_query]) if per_query else np.zeros((0, k), dtype)

    return (np.array([o[0] for o in per_query], dtype=np.uint64), rows_of(1, np.float32), rows_of(2, np.uint32),
            np.array([o[3] for o in per_query], dtype=np.uint64), np.array([o[4] for o in per_query], dtype=np.uint64))


def collapsed_stacked(per_query, k: int, n_groups: int):
    """collapsed_page_after's tuples of a batch -> tests/collapse.py's stacked arrays and, last, skipped u64[n]"""
    return CO.stacked([o[:8] for o in per_query], k, n_groups) + (np.array([o[8] for o in per_query], dtype=np.uint64),)


def last_hit(count, scores, docids):
    """the cursor of the next page: a page's last hit (None: the page is empty)"""
    return (scores[int(count) - 1], int(docids[int(count) - 1])) if int(count) else None


# ---- the cursors of the fuzz cases --------------------------------------------------------------------------------------
def draw_cursor(r, sc, ids, num_docs: int, weights=DRAW_WEIGHTS):
    """One cursor for a query whose matches under the case's mask are (sc, ids), in key order and not empty: with the
    weights' probabilities a uniformly drawn match; a match's score with a random docID in [0, num_docs + 2); from the start
    (None); a random score in (0, 1.1 * the best score) with a random docID."""
    u = r.random()
    if u < weights[0]:
        i = int(r.integers(0, ids.size))
        return sc[i], int(ids[i])
    if u < weights[0] + weights[1]:
        return sc[int(r.integers(0, ids.size))], int(r.integers(0, num_docs + 2))
    if u < weights[0] + weights[1] + weights[2]:
        return None
    s = np.float32(r.random() * 1.1 * float(sc[0]))  # (a best score that underflowed to 0.0: a 0.0 cursor, nothing after it)
    return s, int(r.integers(0, num_docs + 2))


def draw_cursors(seed: int, every, mask, num_docs: int):
    """every: {entry: per query every_match's pair}, in the order the cursors are drawn in -> {entry: per query a cursor}: a
    generator of its own per case, so that the case's base draws do not shift; a query without a match gets no draw (None)."""
    r = np.random.default_rng([seed, DRAW_SEED])
    out = {}
    for entry, per_query in every.items():
        out[entry] = []
        for m in per_query:
            sc, ids = in_filter(m, mask)
            out[entry].append(draw_cursor(r, sc, ids, num_docs) if ids.size else None)
    return out


def split_and_tie(matches, mask, cursor):
    """-> (the cursor splits the matches: 0 < skipped < matches; a match with the cursor's score lies on each side of the cut)"""
    sc, ids = in_filter(matches, mask)
    after = after_cursor(sc, ids, cursor)
    same = sc == _cursor(cursor)[0]
    return bool(0 < after.sum() < ids.size), bool((same & after).any() and (same & ~after).any())
