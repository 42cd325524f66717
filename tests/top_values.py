"""Expected values of the top-values tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py). A match d HAS A VALUE iff
d < len(values); its value is values[d]. Over the n valued matches: distinct, the number of different values, and the first
min(n_top, distinct) of the (value, count) pairs in the order count descending, then value ascending. top_values says this with
np.unique and a lexsort; top_values_by_loop, a document at a time with a dict on Python ints, is what
tests/test_top_values_cpu.py holds it to. Also the named columns of the GPU tests and the draws of the fuzz cases, so that the CPU
tests can replay them without a device."""
import numpy as np

import percentiles as PC

M32 = 0xFFFFFFFF
MAX_TOP = 1024
N_TOPS = (0, 1, 3, 10, 256, 257, 1024)  # the selection's runs are of 256 keys up to 256, of 512 from 257 on, of 1024 at the most
DRAW_SEED = 0x70B5  # the fuzz's generator of columns and n_top: np.random.default_rng([case seed, DRAW_SEED])


def top_values(every, mask, values, n_top: int):
    """-> (n, distinct, top_n, values u32[n_top], counts u32[n_top]); the entries past top_n are 0"""
    v = PC.valued(every, mask, values)
    uniq, cnt = np.unique(v, return_counts=True)
    order = np.lexsort((uniq, -cnt.astype(np.int64)))[:n_top]  # (the last key is the primary one)
    out_v, out_c = np.zeros(n_top, dtype=np.uint32), np.zeros(n_top, dtype=np.uint32)
    out_v[:order.size], out_c[:order.size] = uniq[order], cnt[order]
    return int(v.size), int(uniq.size), int(order.size), out_v, out_c


def top_values_by_loop(every, mask, values, n_top: int):
    """top_values, a document at a time on Python ints"""
    seen, n = {}, 0
    for d in (int(x) for x in every[1]):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        if d < len(values):
            n += 1
            seen[int(values[d])] = seen.get(int(values[d]), 0) + 1
    best = sorted(seen.items(), key=lambda vc: (-vc[1], vc[0]))[:n_top]
    out_v, out_c = np.zeros(n_top, dtype=np.uint32), np.zeros(n_top, dtype=np.uint32)
    for i, (v, c) in enumerate(best):
        out_v[i], out_c[i] = v, c
    return n, len(seen), len(best), out_v, out_c


def stacked(per_query, n_top: int):
    """top_values' tuples of a batch -> the arrays as the binding returns them: (value_counts u64[n], distinct_counts u64[n],
    top_n u32[n], top_values u32[n, n_top], top_counts u32[n, n_top])"""
    n = len(per_query)
    return (np.array([o[0] for o in per_query], dtype=np.uint64), np.array([o[1] for o in per_query], dtype=np.uint64),
            np.array([o[2] for o in per_query], dtype=np.uint32),
            np.stack([o[3] for o in per_query]).reshape(n, n_top) if n else np.zeros((0, n_top), np.uint32),
            np.stack([o[4] for o in per_query]).reshape(n, n_top) if n else np.zeros((0, n_top), np.uint32))


# ---- the named columns --------------------------------------------------------------------------------------------------
def named_columns(top: int, seed: int = 11):
    """The columns of the GPU tests over a docID space of `top` documents, each for a place where the count can go wrong"""
    d = np.arange(top, dtype=np.uint64)
    r = np.random.default_rng(seed)
    return {"all equal": np.full(top, 0x12345678, dtype=np.uint32),  # one word takes every page's add
            "v = d": d.astype(np.uint32),  # all distinct: the order is by value alone, the table at its densest
            "d % 7": (d % 7).astype(np.uint32),  # no two neighbours equal: every run is 1, the page's table does all the merging
            "d // 100": (d // 100).astype(np.uint32),  # runs that cross wave and page boundaries
            "d % 1000": (d % 1000).astype(np.uint32),  # 1 000 values that tie on the every-document list
            # the value whose word has an empty high half, and the value whose inverted key half is 0, in blocks of 300
            "0 and ones": np.where((d // 300) % 2 == 0, 0, M32).astype(np.uint32),
            "wide": r.integers(0, 1 << 32, top, dtype=np.uint64).astype(np.uint32),
            "half": (d[:top // 2] * 3 % 50).astype(np.uint32), "empty": np.zeros(0, dtype=np.uint32)}


# ---- the draws of the fuzz cases ----------------------------------------------------------------------------------------
KINDS = ("few", "many", "all distinct")


def draw_case(seed: int, num_docs: int):
    """One column and one n_top for a case, from a generator of the case's own -> (kind, values, n_top): a column of few values
    (2 to 8), of many (about a third as many as documents, drawn over the whole u32 range) or of a permutation's — every value
    distinct —, in a quarter of the cases cut below the index's docID space; n_top 0 in a tenth of the cases, else with equal
    chance small (1 to 12), around the selection's run sizes (255 to 258, 511 to 513) or the most (1024)."""
    r = np.random.default_rng([seed, DRAW_SEED])
    kind = KINDS[int(r.integers(0, 3))]
    n = max(1, num_docs)
    if kind == "all distinct":  # (times an odd number modulo 2^32: a bijection)
        values = r.permutation(n).astype(np.uint64) * np.uint64(2 * int(r.integers(0, 1 << 31)) + 1) % np.uint64(1 << 32)
    else:
        m = int(r.integers(2, 9)) if kind == "few" else max(1, n // 3)
        values = r.integers(0, 1 << 32, m, dtype=np.uint64)[r.integers(0, m, n)]
    values = values.astype(np.uint32)[:num_docs]
    if r.random() < 0.25:
        values = values[:int(r.integers(0, max(1, num_docs)))]
    u = r.random()
    if u < 0.1:
        n_top = 0
    else:
        pools = (list(range(1, 13)), [255, 256, 257, 258], [511, 512, 513], [1024])
        pool = pools[int(r.integers(0, len(pools)))]
        n_top = int(pool[int(r.integers(0, len(pool)))])
    return kind, values, n_top
