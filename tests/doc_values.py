"""Expected values of the document-values tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py), ordered by a u32 column —
descending or ascending value, equal values by ascending docID in both orders; a document at or past the column's end has
value 0. A match lies AFTER a cursor (cv, cd) iff its value is strictly behind cv in the order, or equal with docID > cd; a
page is the first k of the matches after the cursor, skipped counts the others, and every hit keeps the score the model gives
its document. sorted_page says this with numpy comparisons on (value, docID); sorted_page_by_loop, a document at a time, builds
the device's 64-bit keys K(d) = (ASC ? ~v : v) << 32 | (0xFFFFFFFF - d) and compares integers (tests/test_doc_values_cpu.py
holds the first to it). Also the mask of a value interval, and the column, order and cursor draws of the fuzz cases, so that
the CPU tests can replay them without a device."""
import numpy as np

import doc_filter as DF

DRAW_SEED = 0x50A7  # the fuzz's generator of columns, orders and cursors: np.random.default_rng([case seed, DRAW_SEED])
KINDS = ("few", "wide", "docid", "reverse", "lanes")
W = (0.4, 0.2, 0.1, 0.1, 0.2)
M32 = 0xFFFFFFFF


def value_of(values, ids):
    """v(d) for every d of ids: values[d], 0 at and past len(values)"""
    ids = np.asarray(ids).astype(np.int64)
    out = np.zeros(ids.shape, dtype=np.uint32)
    inside = ids < len(values)
    out[inside] = np.asarray(values, dtype=np.uint32)[ids[inside]]
    return out


def in_order(matches, mask, values, descending: bool):
    """every_match's pair under the mask (None: no filter) in the sorted call's order -> (values u32[m], docids u32[m], scores f32[m])"""
    sc, ids = matches
    if mask is not None:
        keep = DF.holds(mask, ids)
        sc, ids = sc[keep], ids[keep]
    v = value_of(values, ids)
    by = v.astype(np.int64)
    order = np.lexsort((ids, -by if descending else by))
    return v[order], ids[order], sc[order]


def after_cursor(v, ids, descending: bool, cursor):
    """-> bool[m]: which of the documents (v, ids) lie after the cursor (None: every one)"""
    if cursor is None:
        return np.ones(ids.size, dtype=bool)
    cv, cd = int(cursor[0]), int(cursor[1])
    v, d = v.astype(np.int64), ids.astype(np.int64)
    return ((v < cv) if descending else (v > cv)) | ((v == cv) & (d > cd))


def sorted_page(matches, mask, values, descending: bool, cursor, k: int):
    """-> (count, hit_values u32[k], docids u32[k], scores f32[k], matches, skipped), the outputs filled as the device fills
    them: 0 / 0xFFFFFFFF / 0.0 past the count."""
    v, ids, sc = in_order(matches, mask, values, descending)
    after = after_cursor(v, ids, descending, cursor)
    hit_values, docids, scores = np.zeros(k, dtype=np.uint32), np.full(k, M32, dtype=np.uint32), np.zeros(k, dtype=np.float32)
    n = min(int(after.sum()), k)
    hit_values[:n], docids[:n], scores[:n] = v[after][:k], ids[after][:k], sc[after][:k]
    return n, hit_values, docids, scores, int(ids.size), int(ids.size - after.sum())


def key_of(value: int, docid: int, descending: bool) -> int:
    """K: the selection's key of a document, or of a cursor"""
    return (((int(value) if descending else ~int(value)) & M32) << 32) | (M32 - int(docid))


def sorted_page_by_loop(matches, mask, values, descending: bool, cursor, k: int):
    """sorted_page, a document at a time, on the 64-bit integer keys: a document is after a set cursor iff its key is strictly
    below the cursor's; the page is the k largest keys of those, unpacked."""
    ck = None if cursor is None else key_of(cursor[0], cursor[1], descending)
    n, live = 0, []
    for s, d in zip(matches[0], (int(x) for x in matches[1])):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        n += 1
        key = key_of(int(values[d]) if d < len(values) else 0, d, descending)
        assert key != 0
        if ck is None or key < ck:
            live.append((key, s))
    page = sorted(live, key=lambda x: x[0], reverse=True)[:k]
    hit_values, docids, scores = np.zeros(k, dtype=np.uint32), np.full(k, M32, dtype=np.uint32), np.zeros(k, dtype=np.float32)
    for i, (key, s) in enumerate(page):
        hi = key >> 32
        hit_values[i] = hi if descending else (~hi) & M32
        docids[i] = M32 - (key & M32)
        scores[i] = s
    return len(page), hit_values, docids, scores, n, n - len(live)


def values_mask(values, lo: int, hi: int):
    """the bool mask, len(values) entries, of the documents with lo <= v(d) <= hi (closed; lo > hi: nobody)"""
    v = np.asarray(values, dtype=np.uint32).astype(np.int64)
    return (v >= int(lo)) & (v <= int(hi))


def stacked(per_query, k: int):
    """sorted_page's tuples of a batch -> the arrays as the binding returns them: (counts u64[n], hit_values u32[n, k], docids
    u32[n, k], scores f32[n, k], matches u64[n], skipped u64[n])"""
    def rows_of(j, dtype):
        return np.stack([o[j] for o in per_query]) if per_query else np.zeros((0, k), dtype)

    return (np.array([o[0] for o in per_query], dtype=np.uint64), rows_of(1, np.uint32), rows_of(2, np.uint32), rows_of(3, np.float32),
            np.array([o[4] for o in per_query], dtype=np.uint64), np.array([o[5] for o in per_query], dtype=np.uint64))


def last_hit(count, hit_values, docids):
    """the cursor of the next page: (value, docid) of a page's last hit (None: the page is empty)"""
    return (int(hit_values[int(count) - 1]), int(docids[int(count) - 1])) if int(count) else None


# ---- the draws of the fuzz cases ----------------------------------------------------------------------------------------
def fuzz_values(r, n):
    """One column of n documents and an order: few distinct values (ties everywhere), the whole u32 range, the docID, the
    docID reversed, or the lane d & 63; in half of the draws a 0 and a 0xFFFFFFFF planted -> (kind, values u32[n], descending)"""
    kind = KINDS[int(r.choice(len(KINDS), p=W))]
    d = np.arange(n, dtype=np.uint64)
    v = {"few": lambda: r.integers(0, 6, n).astype(np.uint64), "wide": lambda: r.integers(0, 1 << 32, n, dtype=np.uint64),
         "docid": lambda: d, "reverse": lambda: 0xFFFFFFFF - d, "lanes": lambda: d & 63}[kind]().astype(np.uint32)
    if r.random() < 0.5:
        v[int(r.integers(0, n))] = 0
        v[int(r.integers(0, n))] = 0xFFFFFFFF
    return kind, v, bool(r.integers(0, 2))


def draw_cursor(r, v, ids, num_docs: int):
    """One cursor for a query whose matches under the case's mask are (v, ids), not empty: with probability 0.7 a uniformly
    drawn match; 0.1 a match's value with a docID in [0, num_docs + 2); 0.1 none; 0.1 a random u32 value with such a docID."""
    u = r.random()
    if u < 0.7:
        i = int(r.integers(0, ids.size))
        return int(v[i]), int(ids[i])
    if u < 0.8:
        return int(v[int(r.integers(0, ids.size))]), int(r.integers(0, num_docs + 2))
    if u < 0.9:
        return None
    return int(r.integers(0, 1 << 32)), int(r.integers(0, num_docs + 2))


def draw_case(seed: int, every, mask, num_docs: int):
    """every: {entry: per query every_match's pair}, OR's then AND's -> (kind, values u32[num_docs], descending, {entry: per
    query a cursor}), from a generator of the case's own, the column and the order first; a query without a match under the
    mask gets no draw (None). A drawn match is an index into the query's matches under the mask in the SCORE order (descending
    score, equal scores by ascending docID, as tests/paging.py draws its cursors): the figures of
    tests/test_gpu_doc_values_fuzz.py depend on it."""
    r = np.random.default_rng([seed, DRAW_SEED])
    kind, values, descending = fuzz_values(r, num_docs)
    cursors = {}
    for entry, per_query in every.items():
        cursors[entry] = []
        for sc, ids in per_query:
            if mask is not None:
                keep = DF.holds(mask, ids)
                sc, ids = sc[keep], ids[keep]
            ids = ids[np.lexsort((ids, -sc))]
            cursors[entry].append(draw_cursor(r, value_of(values, ids), ids, num_docs) if ids.size else None)
    return kind, values, descending, cursors


def conditions(matches, mask, values, descending: bool, cursor, k: int):
    """The fuzz's four conditions of one (case, query) pair -> (the from-the-start page's docID set differs from the
    score-ranked top k's; the value of hit k equals the value of the first match left out; the cursor splits the matches; a
    match with the cursor's value lies on each side of the cut; matches > k)"""
    v, ids, _ = in_order(matches, mask, values, descending)
    sc, all_ids = matches
    if mask is not None:
        keep = DF.holds(mask, all_ids)
        sc, all_ids = sc[keep], all_ids[keep]
    by_score = all_ids[np.lexsort((all_ids, -sc))[:k]]
    differs = set(ids[:k].tolist()) != set(by_score.tolist())
    tie_at_cut = bool(ids.size > k and v[k - 1] == v[k])
    after = after_cursor(v, ids, descending, cursor)
    splits = bool(0 < after.sum() < ids.size)
    same = (v == (cursor[0] if cursor is not None else -1)) if cursor is not None else np.zeros(ids.size, dtype=bool)
    return differs, tie_at_cut, splits, bool((same & after).any() and (same & ~after).any()), bool(ids.size > k)
