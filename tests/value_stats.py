"""Expected values of the value-stats tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py). A match d HAS A VALUE iff
d < len(values); its value is values[d]. Over the valued matches: n, the sum, the minimum and the maximum — (0, 0, 0xFFFFFFFF, 0)
where there is none — and, with edges, the row of n_edges + 1 buckets, bucket(v) = the number of edges e with e <= v. The hit
values are the values of the filtered call's top k (0 past the count and for a hit without a value). value_stats says this with
numpy (searchsorted side="right", bincount); value_stats_by_loop, a document at a time on Python ints, is what
tests/test_value_stats_cpu.py holds it to. Also the named edge sets and columns of the GPU tests and the draws of the fuzz cases,
so that the CPU tests can replay them without a device."""
import numpy as np

import doc_filter as DF
import doc_values as DV

M32 = 0xFFFFFFFF
MAX_EDGES = 1023
EMPTY = (0, 0, M32, 0)
STATS_DTYPE = np.dtype([("n", np.uint64), ("sum", np.uint64), ("min", np.uint32), ("max", np.uint32)])
DRAW_SEED = 0x57A7  # the fuzz's generator of columns and edges: np.random.default_rng([case seed, DRAW_SEED])


def matches_in(matches, mask):
    """every_match's pair under the mask (None: no filter) -> (scores, docids)"""
    sc, ids = matches
    if mask is None:
        return sc, ids
    keep = DF.holds(mask, ids)
    return sc[keep], ids[keep]


def value_stats(matches, mask, values, edges, k: int):
    """-> ((n, sum, min, max) as Python ints, the bucket row u32[n_edges + 1] — None without edges —, hit_values u32[k])"""
    sc, ids = matches_in(matches, mask)
    values = np.asarray(values, dtype=np.uint32)
    v = values[ids[ids.astype(np.int64) < values.size].astype(np.int64)].astype(np.uint64)
    stats = (int(v.size), int(v.sum(dtype=np.uint64)), int(v.min()), int(v.max())) if v.size else EMPTY
    row = None
    if edges is not None and len(edges):
        e = np.asarray(edges, dtype=np.uint64)
        row = np.bincount(np.searchsorted(e, v, side="right"), minlength=e.size + 1).astype(np.uint32)
    best = np.lexsort((ids, -sc))[:k]
    hit_values = np.zeros(k, dtype=np.uint32)
    hit_values[:best.size] = DV.value_of(values, ids[best])
    return stats, row, hit_values


def value_stats_by_loop(matches, mask, values, edges, k: int):
    """value_stats, a document at a time on Python ints"""
    n = total = 0
    lo, hi = M32, 0
    n_edges = 0 if edges is None else len(edges)
    row = [0] * (n_edges + 1)
    live = []
    for s, d in zip(matches[0], (int(x) for x in matches[1])):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        live.append((-float(s), d))
        if d >= len(values):
            continue
        v = int(values[d])
        n, total, lo, hi = n + 1, total + v, min(lo, v), max(hi, v)
        row[sum(1 for e in edges if int(e) <= v) if n_edges else 0] += 1
    hit_values = np.zeros(k, dtype=np.uint32)
    for i, (_, d) in enumerate(sorted(live)[:k]):
        hit_values[i] = int(values[d]) if d < len(values) else 0
    return (n, total, lo, hi), (np.array(row, dtype=np.uint32) if n_edges else None), hit_values


def stacked(per_query, k: int, n_edges: int):
    """value_stats' tuples of a batch -> the arrays as the binding returns them: (stats STATS_DTYPE[n], buckets
    u32[n, n_edges + 1] or None, hit_values u32[n, k])"""
    stats = np.array([o[0] for o in per_query], dtype=STATS_DTYPE) if per_query else np.zeros(0, dtype=STATS_DTYPE)
    buckets = None
    if n_edges:
        buckets = np.stack([o[1] for o in per_query]) if per_query else np.zeros((0, n_edges + 1), np.uint32)
    return stats, buckets, np.stack([o[2] for o in per_query]) if per_query else np.zeros((0, k), np.uint32)


# ---- the named edge sets and columns ------------------------------------------------------------------------------------
def evenly(n_edges: int, lo: int, hi: int):
    """n_edges strictly ascending edges over [lo, hi], both ends among them where n_edges >= 2"""
    assert hi - lo + 1 >= n_edges
    return np.unique(np.linspace(lo, hi, n_edges).astype(np.uint64)).astype(np.uint32) if n_edges > 1 else np.array([lo][:n_edges], dtype=np.uint32)


def edge_sets(values):
    """The edge sets of the CPU model test over a column: none, the two ends alone and together, an edge that equals a present
    value (and its two neighbours), and the most a call takes."""
    present = int(np.asarray(values)[len(values) // 2]) if len(values) else 5
    around = sorted({max(0, present - 1), present, min(M32, present + 1)})
    return {"none": [], "0": [0], "the top": [M32], "both ends": [0, M32], "a present value": [present], "around it": around,
            "1023": evenly(MAX_EDGES, 0, M32).tolist()}


def named_columns(top: int, seed: int = 11):
    """The columns of the GPU tests over a docID space of `top` documents"""
    d = np.arange(top, dtype=np.uint64)
    r = np.random.default_rng(seed)
    return {"zeros": np.zeros(top, dtype=np.uint32), "ones": np.full(top, M32, dtype=np.uint32), "v = d": d.astype(np.uint32),
            "reverse": (M32 - d).astype(np.uint32), "wide": r.integers(0, 1 << 32, top, dtype=np.uint64).astype(np.uint32),
            "half": (d[:top // 2] * 3).astype(np.uint32), "top + 3": (d.max() + 3 - np.arange(top + 3, dtype=np.uint64)).astype(np.uint32),
            "empty": np.zeros(0, dtype=np.uint32)}


# ---- the draws of the fuzz cases ----------------------------------------------------------------------------------------
EDGE_COUNTS = ("none", "1-8", "9-300", "1023")
EDGE_WEIGHTS = (0.1, 0.3, 0.35, 0.25)


def fuzz_edges(r, values):
    """One edge set for a column: a count among 0 / 1-8 / 9-300 / 1023, the edges a third each from the column's present values,
    from their neighbours (value - 1, value + 1) and uniformly from the u32 range, made unique and ascending (so a drawn count
    is an upper bound but for 1023, which is topped up uniformly) -> (which count, edges u32[n_edges])"""
    which = EDGE_COUNTS[int(r.choice(len(EDGE_COUNTS), p=EDGE_WEIGHTS))]
    want = {"none": 0, "1-8": int(r.integers(1, 9)), "9-300": int(r.integers(9, 301)), "1023": MAX_EDGES}[which]
    if want == 0:
        return which, np.zeros(0, dtype=np.uint32)
    pool = [r.integers(0, 1 << 32, want, dtype=np.uint64)]
    if len(values):
        at = np.asarray(values, dtype=np.uint64)[r.integers(0, len(values), want)]
        pool += [at, np.clip(at.astype(np.int64) + r.choice([-1, 1], want), 0, M32).astype(np.uint64)]
    e = np.unique(r.permutation(np.concatenate(pool))[:want])
    while which == "1023" and e.size < want:
        e = np.unique(np.concatenate([e, r.integers(0, 1 << 32, want - e.size, dtype=np.uint64)]))
    return which, e.astype(np.uint32)


def draw_case(seed: int, num_docs: int):
    """-> (kind, values, which count, edges) from a generator of the case's own: the column as tests/doc_values.py's fuzz_values
    draws it, in a quarter of the cases cut to a length below the index's docID space (a short column), in a tenth two
    documents longer; then the edges."""
    r = np.random.default_rng([seed, DRAW_SEED])
    u = r.random()
    n_col = int(r.integers(0, num_docs)) if u < 0.25 else num_docs + 2 if u < 0.35 else num_docs
    kind, values, _ = DV.fuzz_values(r, max(1, n_col))
    values = values[:n_col]
    which, edges = fuzz_edges(r, values)
    return kind, values, which, edges


def conditions(per_query, n_col: int, num_docs: int, n_edges: int):
    """The fuzz's four conditions of one (case, entry) -> (more than 256 buckets, a short column, some query's sum at or above
    2^32, some query with more than 256 valued matches — more than a page holds, so its record and row meet across pages);
    per_query: value_stats' tuples"""
    return (n_edges + 1 > 256, n_col < num_docs, any(o[0][1] >= 1 << 32 for o in per_query), any(o[0][0] > 256 for o in per_query))
