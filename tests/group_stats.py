"""Expected values of the group-stats tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py). A match d is IN GROUP g
iff d < len(group_of) and group_of[d] == g (tests/facets.py: NONE is no group); it HAS A VALUE iff d < len(values)
(tests/doc_values.py). Per group g < n_groups, over the matches in g that have a value: n, the sum, the minimum and the maximum —
(0, 0, 0xFFFFFFFF, 0) where there is none. A match in no group contributes nowhere, and so does a match in a group but past the
column. group_stats says this with numpy (bincount, minimum.at, maximum.at); group_stats_by_loop, a document at a time on Python
ints, is what tests/test_group_stats_cpu.py holds it to. Also the named cases of the GPU tests and the draws of the fuzz cases, so
that the CPU test can replay them without a device."""
import numpy as np

import doc_filter as DF
import doc_values as DV
import facets as FA
import value_stats as VS
from ranked_range import every_match  # noqa: F401  (the matches every model here starts from)

M32 = 0xFFFFFFFF
EMPTY = VS.EMPTY
STATS_DTYPE = VS.STATS_DTYPE
DRAW_SEED = 0x6A57  # the fuzz's generator of maps and columns: np.random.default_rng([case seed, DRAW_SEED])


def matches_in(matches, mask):
    """every_match's pair -> the docIDs under the mask (None: no filter)"""
    return FA.matches_in(matches, mask)


def group_stats(matches, mask, group_of, n_groups: int, values):
    """-> STATS_DTYPE[n_groups]: the records of one query"""
    ids = matches_in(matches, mask).astype(np.int64)
    values = np.asarray(values, dtype=np.uint32)
    g = FA.groups_of(group_of, ids)
    use = (g != FA.NONE) & (ids < values.size)
    g, v = g[use], values[ids[use]].astype(np.uint64)
    out = np.zeros(n_groups, dtype=STATS_DTYPE)
    out["n"] = np.bincount(g, minlength=n_groups)
    lo, hi = v & np.uint64(0xFFFF), v >> np.uint64(16)  # (bincount's weights are doubles: the halves stay exact)
    out["sum"] = (np.bincount(g, weights=hi, minlength=n_groups).astype(np.uint64) << np.uint64(16)) + \
        np.bincount(g, weights=lo, minlength=n_groups).astype(np.uint64)
    mn, mx = np.full(n_groups, M32, dtype=np.uint32), np.zeros(n_groups, dtype=np.uint32)
    np.minimum.at(mn, g, v.astype(np.uint32))
    np.maximum.at(mx, g, v.astype(np.uint32))
    out["min"], out["max"] = mn, mx
    return out


def group_stats_by_loop(matches, mask, group_of, n_groups: int, values):
    """group_stats, a document at a time on Python ints"""
    recs = [list(EMPTY) for _ in range(n_groups)]
    for d in (int(x) for x in matches[1]):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        g = int(group_of[d]) if d < len(group_of) else FA.NONE
        if g == FA.NONE or d >= len(values):
            continue
        v, r = int(values[d]), recs[g]
        r[0], r[1], r[2], r[3] = r[0] + 1, r[1] + v, min(r[2], v), max(r[3], v)
    return np.array([tuple(r) for r in recs], dtype=STATS_DTYPE)


def stacked(per_query, n_groups: int):
    """group_stats' records of a batch -> STATS_DTYPE[n, n_groups], as the binding returns them"""
    return np.stack(per_query) if per_query else np.zeros((0, n_groups), dtype=STATS_DTYPE)


def empty_records(n: int, n_groups: int):
    return np.full((n, n_groups), np.array([EMPTY], dtype=STATS_DTYPE)[0], dtype=STATS_DTYPE)


# ---- the named cases ----------------------------------------------------------------------------------------------------
GROUP_COUNTS = (1, 2, 255, 256, 257, 300, 65536)  # the LDS table against direct atomics, and bin t past n_groups
COLUMNS = ("zeros", "ones", "half", "top + 3", "empty", "wide")
named_columns = VS.named_columns


def named_maps(num_docs: int, n_groups: int):
    """FA.MAPS over num_docs documents, a map shorter than the index and one longer (both clustered), a map whose document 0
    holds group 0 alone (lane 0 of the first page; no other page sees group 0), and a clustered map whose rows of 16 hold
    runs of 5 (runs that cross the row boundaries 16 / 32 / 48) -> {name: int64 map}"""
    maps = {name: FA.named_map(name, num_docs, n_groups) for name in FA.MAPS}
    maps["short"] = FA.named_map("clustered", num_docs // 2 + 3, n_groups)
    maps["long"] = FA.named_map("clustered", num_docs + 70, n_groups)
    lone = np.full(num_docs, n_groups - 1, dtype=np.int64)
    lone[0] = 0
    maps["group 0 in lane 0 only"] = lone
    maps["runs of 5"] = (np.arange(num_docs, dtype=np.int64) // 5) % n_groups
    return maps


# ---- the draws of the fuzz cases ----------------------------------------------------------------------------------------
def draw_case(seed: int, num_docs: int):
    """-> (map kind, n_groups, group_of, column kind, values) from a generator of the case's own: the map as tests/facets.py's
    fuzz_map draws it (its length below, at or above the index's docID space) — in a quarter of the cases with at most 3 groups
    instead of its draw, so that a group gathers more matches than a page holds —, then the column as tests/doc_values.py's
    fuzz_values draws it, in a quarter of the cases cut to a length below the index's docID space (a short column), in a tenth
    two documents longer."""
    r = np.random.default_rng([seed, DRAW_SEED])
    map_kind, n_groups, group_of = FA.fuzz_map(r, num_docs)
    if r.random() < 0.25:
        n_groups = int(r.integers(1, 4))
        group_of = FA.named_map(map_kind, len(group_of), n_groups, seed=seed)
    u = r.random()
    n_col = int(r.integers(0, num_docs)) if u < 0.25 else num_docs + 2 if u < 0.35 else num_docs
    col_kind, values, _ = DV.fuzz_values(r, max(1, n_col))
    return map_kind, n_groups, group_of, col_kind, values[:n_col]


CONDITIONS = ("more than 256 groups", "at most 256 groups", "a short column", "a short map", "a (query, group) sum >= 2^32",
              "a (query, group) with more than 256 contributing matches")


def conditions(per_query, n_groups: int, n_map: int, n_col: int, num_docs: int):
    """The fuzz's conditions of one (case, entry), in CONDITIONS' order -> a tuple of bools; per_query: group_stats' records"""
    recs = stacked(per_query, n_groups)
    return (n_groups > 256, n_groups <= 256, n_col < num_docs, n_map < num_docs, bool((recs["sum"] >= 1 << 32).any()),
            bool((recs["n"] > 256).any()))
