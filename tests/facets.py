"""Expected values of the faceted ranked tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py), and the facet row is
numpy.bincount over the matches' groups: group_of[d] for d < len(group_of), none past it, NONE (-1 here, 0xFFFFFFFF on the
device) for a document in no group. Also the named group maps of the handle, batch and fuzz tests, so that
tests/test_facets_cpu.py can replay them without a device."""
import numpy as np

import doc_filter as DF

NONE = -1  # a document in no group, as the model and DocFacets' input have it
every_match = DF.every_match


def groups_of(group_of, ids):
    """group_of[ids], NONE at and past len(group_of) -> int64"""
    group_of = np.asarray(group_of, dtype=np.int64)
    ids = np.asarray(ids).astype(np.int64)
    out = np.full(ids.shape, NONE, dtype=np.int64)
    inside = ids < group_of.size
    out[inside] = group_of[ids[inside]]
    return out


def row_of(group_of, n_groups: int, ids):
    """the facet row of the matches `ids` -> (row u32[n_groups], the matches in no group)"""
    g = groups_of(group_of, ids)
    real = g[g != NONE]
    return np.bincount(real, minlength=n_groups).astype(np.uint32), int(g.size - real.size)


def matches_in(matches, mask):
    """every_match's pair -> the docIDs in the filter (mask None: all of them)"""
    ids = matches[1]
    return ids if mask is None else ids[DF.holds(mask, ids)]


def row_by_loop(group_of, n_groups: int, ids):
    """row_of, a document at a time (tests/test_facets_cpu.py holds row_of to it)"""
    row, none = [0] * n_groups, 0
    for d in (int(x) for x in ids):
        g = int(group_of[d]) if d < len(group_of) else NONE
        if g == NONE:
            none += 1
        else:
            row[g] += 1
    return np.array(row, dtype=np.uint32), none


def sizes_of(group_of, n_groups: int):
    """the handle's group_sizes and n_grouped"""
    g = np.asarray(group_of, dtype=np.int64)
    sizes = np.bincount(g[g != NONE], minlength=n_groups).astype(np.uint32)
    return sizes, int(sizes.sum())


# ---- the named maps -----------------------------------------------------------------------------------------------------
MAPS = ("clustered", "striped", "random", "one group", "none", "every other document NONE")


def named_map(name: str, num_docs: int, n_groups: int, seed: int = 7):
    """-> int64[num_docs] with values in [0, n_groups) or NONE. clustered: d // w, the groups consecutive runs of equal
    width (the last group takes the rest); striped: d % n_groups; random: uniform; one group: every document in the LAST
    group; none: no document in a group; every other document NONE: clustered, the odd documents in no group."""
    d = np.arange(num_docs, dtype=np.int64)
    w = max(1, -(-num_docs // n_groups))
    if name == "clustered":
        return np.minimum(d // w, n_groups - 1)
    if name == "striped":
        return d % n_groups
    if name == "random":
        return np.random.default_rng(seed).integers(0, n_groups, num_docs).astype(np.int64)
    if name == "one group":
        return np.full(num_docs, n_groups - 1, dtype=np.int64)
    if name == "none":
        return np.full(num_docs, NONE, dtype=np.int64)
    if name == "every other document NONE":
        return np.where(d & 1, NONE, np.minimum(d // w, n_groups - 1))
    raise ValueError(name)


# ---- the maps of the fuzz cases -----------------------------------------------------------------------------------------
FUZZ_WEIGHTS = (0.3, 0.25, 0.25, 0.04, 0.04, 0.12)  # of MAPS, in order


def fuzz_map(r, top: int):
    """One seeded map of a random kind for an index whose largest docID is top - 1 -> (kind, n_groups, group_of). n_groups is
    drawn from 1 .. 600 — half of the draws at most 256, the LDS form, half above, the global form — and the map's length
    below, at and above the index's largest docID + 1."""
    n_groups = int(r.integers(1, 257)) if r.random() < 0.5 else int(r.integers(257, 601))
    num_docs = max(1, int(top * r.choice([0.5, 0.9, 1.0, 1.0, 1.0, 1.3])) + int(r.integers(0, 3)))
    kind = MAPS[int(r.choice(len(MAPS), p=FUZZ_WEIGHTS))]
    return kind, n_groups, named_map(kind, num_docs, n_groups, seed=int(r.integers(0, 1 << 30)))
