"""Expected values of the group-limited ranked tests: a query's matches are the unfiltered
model's (tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py), and grouped by
tests/facets.py's groups_of. One lexsort by (-score, docID) — the device's key order: a higher score first, equal scores by
ascending docID — puts every group's documents in the group's own key order, so a document's rank within its group is a
running count along that order. The kept documents are those of rank < per_group plus every document in no group; the
cursor (tests/paging.py) cuts the kept documents on the keys' integers, and the page is the first k of what lies after it.
Also the per_group draw of the fuzz cases, so that tests/test_group_limit_cpu.py can replay them without a device."""
import numpy as np

import collapse as CO
import doc_filter as DF
import facets as FA
import paging as PG

NONE = FA.NONE
DEVICE_NONE = CO.DEVICE_NONE
MAX = 16  # DINT_GROUP_LIMIT_MAX
every_match = FA.every_match
PER_GROUP_SEED = 0x61C7
PER_GROUP_CHOICES = (1, 2, 2, 3, 3, 4, 8, 16)


def fuzz_per_group(case_seed: int) -> int:
    """the per_group of a fuzz case: a generator of its own per case, so that the case's base draws do not shift"""
    return int(np.random.default_rng([case_seed, PER_GROUP_SEED]).choice(PER_GROUP_CHOICES))


def keys_of(sc, ids):
    """the selection's keys of documents as integers: the score's bits, then the inverted docID -> u64[m]"""
    bits = np.ascontiguousarray(sc, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (bits << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids).astype(np.uint64))


def ranked_in_groups(matches, mask, group_of):
    """every_match's pair under the mask, in key order -> (scores, docids, groups, ranks): ranks[i] the 0-based position of
    document i among the matches of its group in key order (0 for a document in no group)"""
    sc, ids = PG.in_filter(matches, mask)
    g = FA.groups_of(group_of, ids)
    ranks = np.zeros(ids.size, dtype=np.int64)
    by_group = np.argsort(g, kind="stable")  # (stable: within a group the key order stays)
    gs = g[by_group]
    starts = np.flatnonzero(np.r_[True, gs[1:] != gs[:-1]]) if ids.size else np.zeros(0, dtype=np.int64)
    run_start = np.repeat(starts, np.diff(np.r_[starts, ids.size]))
    ranks[by_group] = np.arange(ids.size) - run_start
    ranks[g == NONE] = 0
    return sc, ids, g, ranks


def group_limit(matches, mask, group_of, n_groups: int, k: int, per_group: int, after=None):
    """every_match's pair, the filter's mask (None: no filter), the map, and the cursor (None: from the start) -> (count,
    scores f32[k], docids u32[k], matches, kept, hit_groups u32[k], hit_group_matches u32[k], hit_group_ranks u32[k], row
    u32[n_groups], skipped), the outputs filled as the device fills them: 0.0 / 0xFFFFFFFF / DEVICE_NONE / 0 / 0 past the
    count."""
    assert 1 <= per_group <= MAX
    sc, ids, g, ranks = ranked_in_groups(matches, mask, group_of)
    row = np.bincount(g[g != NONE], minlength=n_groups).astype(np.uint32)
    kept = np.flatnonzero((ranks < per_group) | (g == NONE))
    ck = PG.cursor_key(after)
    behind = kept[keys_of(sc[kept], ids[kept]) < np.uint64(ck)] if ck != PG.FROM_START else kept
    best = behind[:k]
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    hit_groups = np.full(k, DEVICE_NONE, dtype=np.uint32)
    hit_group_matches = np.zeros(k, dtype=np.uint32)
    hit_group_ranks = np.zeros(k, dtype=np.uint32)
    scores[:best.size] = sc[best]
    docids[:best.size] = ids[best]
    gb = g[best]
    hit_groups[:best.size] = np.where(gb == NONE, DEVICE_NONE, gb).astype(np.uint32)
    hit_group_matches[:best.size] = np.where(gb == NONE, 1, row[np.where(gb == NONE, 0, gb)])
    hit_group_ranks[:best.size] = ranks[best]
    return (best.size, scores, docids, int(ids.size), int(kept.size), hit_groups, hit_group_matches, hit_group_ranks, row,
            int(kept.size - behind.size))


def group_limit_by_loop(matches, mask, group_of, n_groups: int, k: int, per_group: int, after=None):
    """group_limit, a document at a time on Python values: every group's (key, docID) pairs in a list, its per_group largest
    kept with their positions, the ungrouped documents on their own, the cursor on the keys' integers, then a sort."""
    groups, loose, row, n = {}, [], [0] * n_groups, 0
    for s, d in zip(matches[0], (int(x) for x in matches[1])):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        n += 1
        g = int(group_of[d]) if d < len(group_of) else NONE
        if g == NONE:
            loose.append((PG.key_of(s, d), s, d, g, 0))
            continue
        row[g] += 1
        groups.setdefault(g, []).append((PG.key_of(s, d), s, d))
    kept = list(loose)
    for g, docs in groups.items():
        docs.sort(reverse=True)
        kept += [(key, s, d, g, r) for r, (key, s, d) in enumerate(docs[:per_group])]
    kept.sort(reverse=True)
    ck = PG.cursor_key(after)
    behind = [x for x in kept if x[0] < ck]
    scores = np.zeros(k, dtype=np.float32)
    docids = np.full(k, 0xFFFFFFFF, dtype=np.uint32)
    hit_groups = np.full(k, DEVICE_NONE, dtype=np.uint32)
    hit_group_matches = np.zeros(k, dtype=np.uint32)
    hit_group_ranks = np.zeros(k, dtype=np.uint32)
    for i, (_, s, d, g, r) in enumerate(behind[:k]):
        scores[i], docids[i] = s, d
        hit_groups[i] = DEVICE_NONE if g == NONE else g
        hit_group_matches[i] = 1 if g == NONE else row[g]
        hit_group_ranks[i] = r
    return (min(len(behind), k), scores, docids, n, len(kept), hit_groups, hit_group_matches, hit_group_ranks,
            np.array(row, dtype=np.uint32), len(kept) - len(behind))


def stacked(per_query, k: int, n_groups: int):
    """group_limit's tuples of a batch -> the arrays as the binding returns them with_stats (without blocks_decoded) and
    with_rows: (counts u64[n], scores f32[n, k], docids u32[n, k], matches u64[n], kept u64[n], hit_groups u32[n, k],
    hit_group_matches u32[n, k], hit_group_ranks u32[n, k], rows u32[n, n_groups], skipped u64[n])"""
    def rows_of(j, width, dtype):
        return np.stack([o[j] for o in per_query]) if per_query else np.zeros((0, width), dtype)

    def column(j):
        return np.array([o[j] for o in per_query], dtype=np.uint64)

    return (column(0), rows_of(1, k, np.float32), rows_of(2, k, np.uint32), column(3), column(4), rows_of(5, k, np.uint32),
            rows_of(6, k, np.uint32), rows_of(7, k, np.uint32), rows_of(8, n_groups, np.uint32), column(9))


def whole_order(matches, mask, group_of, n_groups: int, per_group: int):
    """every kept document of a query in key order -> (scores, docids, hit_groups, hit_group_matches, hit_group_ranks): what
    a walk from the start must show, page after page"""
    k_all = max(1, int(matches[1].size))
    n, sc, ids, _, kept, groups, group_matches, ranks, _, _ = group_limit(matches, mask, group_of, n_groups, k_all, per_group)
    assert n == kept
    return sc[:n], ids[:n], groups[:n], group_matches[:n], ranks[:n]


def conditions(matches, mask, group_of, per_group: int):
    """what the fuzz requires of its cases, of one (case, query) -> (kept < matches: some group was cut; a group's second or
    later match is kept; a group's places per_group and per_group + 1 hold equal scores: a tie across the cut)"""
    sc, ids, g, ranks = ranked_in_groups(matches, mask, group_of)
    grouped = g != NONE
    kept = (ranks < per_group) | ~grouped
    last_in, first_out = grouped & (ranks == per_group - 1), grouped & (ranks == per_group)
    tie = False
    if first_out.any():
        score_in = dict(zip(g[last_in].tolist(), sc[last_in].tolist()))
        tie = any(score_in[gg] == s for gg, s in zip(g[first_out].tolist(), sc[first_out].tolist()))
    return bool(kept.sum() < ids.size), bool((grouped & kept & (ranks >= 1)).any()), bool(tie)
