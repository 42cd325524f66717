"""Expected values of the collapsed ranked tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py), and grouped by
tests/facets.py's groups_of. One lexsort by (-score, docID) — the device's key order: a higher score first, equal scores by
ascending docID — puts every group's best document in front of the group's others, so the kept documents are the first of
every group in that order plus every document in no group, and the top k are the first k of them. Also the map generator of
the fuzz cases, so that tests/test_collapse_cpu.py can replay them without a device."""
import numpy as np

import doc_filter as DF
import facets as FA

NONE = FA.NONE
DEVICE_NONE = 0xFFFFFFFF  # DINT_FACET_NONE, as hit_groups carries it
every_match = FA.every_match


def collapse(matches, mask, group_of, n_groups: int, k: int):
    """every_match's pair, the filter's mask (None: no filter) and the map -> (count, scores f32[k], docids u32[k],
    matches, collapsed, hit_groups u32[k], hit_group_matches u32[k], row u32[n_groups]), the outputs filled as the device
    fills them: 0.0 / 0xFFFFFFFF / DEVICE_NONE / 0 past the count."""
    sc, ids = matches
    if mask is not None:
        keep = DF.holds(mask, ids)
        sc, ids = sc[keep], ids[keep]
    order = np.lexsort((ids, -sc))
    sc, ids = sc[order], ids[order]
    g = FA.groups_of(group_of, ids)
    row = np.bincount(g[g != NONE], minlength=n_groups).astype(np.uint32)
    first = np.zeros(ids.size, dtype=bool)  # the first document of its group in key order
    first[np.unique(g, return_index=True)[1]] = True
    kept = np.flatnonzero(first | (g == NONE))
    best = kept[:k]
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    hit_groups = np.full(k, DEVICE_NONE, dtype=np.uint32)
    hit_group_matches = np.zeros(k, dtype=np.uint32)
    scores[:best.size] = sc[best]
    docids[:best.size] = ids[best]
    gb = g[best]
    hit_groups[:best.size] = np.where(gb == NONE, DEVICE_NONE, gb).astype(np.uint32)
    hit_group_matches[:best.size] = np.where(gb == NONE, 1, row[np.where(gb == NONE, 0, gb)])
    return best.size, scores, docids, int(ids.size), int(kept.size), hit_groups, hit_group_matches, row


def collapse_by_loop(matches, mask, group_of, n_groups: int, k: int):
    """collapse, a document at a time (tests/test_collapse_cpu.py holds collapse to it): the best (score, -docID) of every
    group in a dictionary, the ungrouped documents on their own, then a sort of what is left."""
    best, loose, row, n = {}, [], [0] * n_groups, 0
    for s, d in zip(matches[0], (int(x) for x in matches[1])):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        n += 1
        g = int(group_of[d]) if d < len(group_of) else NONE
        if g == NONE:
            loose.append((s, d, g))
            continue
        row[g] += 1
        if g not in best or (s, -d) > (best[g][0], -best[g][1]):
            best[g] = (s, d, g)
    kept = sorted(list(best.values()) + loose, key=lambda x: (-float(x[0]), x[1]))
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    hit_groups = np.full(k, DEVICE_NONE, dtype=np.uint32)
    hit_group_matches = np.zeros(k, dtype=np.uint32)
    for i, (s, d, g) in enumerate(kept[:k]):
        scores[i], docids[i] = s, d
        hit_groups[i] = DEVICE_NONE if g == NONE else g
        hit_group_matches[i] = 1 if g == NONE else row[g]
    return min(len(kept), k), scores, docids, n, len(kept), hit_groups, hit_group_matches, np.array(row, dtype=np.uint32)


def stacked(per_query, k: int, n_groups: int):
    """collapse's tuples of a batch -> the arrays as the binding returns them: (counts u64[n], scores f32[n, k], docids
    u32[n, k], matches u64[n], collapsed u64[n], hit_groups u32[n, k], hit_group_matches u32[n, k], rows u32[n, n_groups])"""
    def rows_of(j, width, dtype):
        return np.stack([o[j] for o in per_query]) if per_query else np.zeros((0, width), dtype)

    return (np.array([o[0] for o in per_query], dtype=np.uint64), rows_of(1, k, np.float32), rows_of(2, k, np.uint32),
            np.array([o[3] for o in per_query], dtype=np.uint64), np.array([o[4] for o in per_query], dtype=np.uint64),
            rows_of(5, k, np.uint32), rows_of(6, k, np.uint32), rows_of(7, n_groups, np.uint32))


# ---- the maps of the fuzz cases -----------------------------------------------------------------------------------------
# Few groups and clustered kinds weigh most: with a group per few documents a query's matches seldom share a group and
# collapsing removes nothing, and under "one group" or "none" either nothing is removed or a single document is kept.
FUZZ_WEIGHTS = (0.4, 0.22, 0.22, 0.04, 0.04, 0.08)  # of FA.MAPS, in order


def fuzz_map(r, top: int):
    """One seeded map of a random kind for an index whose largest docID is top - 1 -> (kind, n_groups, group_of). n_groups in
    1 .. 600: three draws in five at most 24 (matches share groups), one in 25 .. 256 (the LDS form still), one in
    257 .. 600 (the global form); the map's length below, at and above the index's largest docID + 1."""
    u = r.random()
    n_groups = int(r.integers(2, 25)) if u < 0.6 else int(r.integers(1, 257)) if u < 0.75 else int(r.integers(257, 601))
    num_docs = max(1, int(top * r.choice([0.5, 0.9, 1.0, 1.0, 1.0, 1.3])) + int(r.integers(0, 3)))
    kind = FA.MAPS[int(r.choice(len(FA.MAPS), p=FUZZ_WEIGHTS))]
    return kind, n_groups, FA.named_map(kind, num_docs, n_groups, seed=int(r.integers(0, 1 << 30)))
