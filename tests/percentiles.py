"""Expected values of the percentile tests: a query's matches are the unfiltered model's
(tests/ranked_range.py's every_match), kept where the filter's mask holds them (tests/doc_filter.py). A match d HAS A VALUE iff
d < len(values); its value is values[d]. With s the ascending sort of the n valued matches' values, duplicates kept, the answer
to per_million[j] is s[((n - 1) * per_million[j]) // 1000000] — the lower nearest rank, the index computed on Python ints — and
0 where n == 0. percentiles says this with np.sort; percentiles_by_loop, a document at a time with sorted() on Python ints, is
what tests/test_percentiles_cpu.py holds it to. Also the named columns and percentile sets of the GPU tests and the draws of the
fuzz cases, so that the CPU tests can replay them without a device."""
import numpy as np

import value_stats as VS

M32 = 0xFFFFFFFF
MILLION = 1000000
MAX_PERCENTILES = 16
MAX_RECORDS = 1 << 16
DRAW_SEED = 0x9C71  # the fuzz's generator of percentile sets: np.random.default_rng([case seed, DRAW_SEED])


def rank_of(n: int, per_million: int) -> int:
    """the index into the ascending sort of n values (n >= 1), on Python ints"""
    return ((int(n) - 1) * int(per_million)) // MILLION


def valued(matches, mask, values):
    """-> the values of the matches under the mask that have one, in docID order, u32"""
    ids = VS.matches_in(matches, mask)[1].astype(np.int64)
    values = np.asarray(values, dtype=np.uint32)
    return values[ids[ids < values.size]]


def percentiles(every, mask, values, per_million):
    """-> (n, the answers u32[len(per_million)])"""
    s = np.sort(valued(every, mask, values))
    n = int(s.size)
    return n, np.array([int(s[rank_of(n, p)]) if n else 0 for p in per_million], dtype=np.uint32)


def percentiles_by_loop(every, mask, values, per_million):
    """percentiles, a document at a time on Python ints"""
    have = []
    for d in (int(x) for x in every[1]):
        if mask is not None and not (d < len(mask) and mask[d]):
            continue
        if d < len(values):
            have.append(int(values[d]))
    have = sorted(have)
    out = np.zeros(len(per_million), dtype=np.uint32)
    for j, p in enumerate(per_million):
        if have:
            out[j] = have[((len(have) - 1) * int(p)) // 1000000]
    return len(have), out


def stacked(per_query, n_percentiles: int):
    """percentiles' tuples of a batch -> the arrays as the binding returns them: (value_counts u64[n], values u32[n, n_percentiles])"""
    counts = np.array([o[0] for o in per_query], dtype=np.uint64)
    return counts, np.stack([o[1] for o in per_query]) if per_query else np.zeros((0, n_percentiles), np.uint32)


def percents(per_million):
    """parts per million -> the percents the binding takes (it converts by round(p * 10000), which gives these back)"""
    return [int(p) / 10000 for p in per_million]


# ---- the named columns and percentile sets ------------------------------------------------------------------------------
HALF_LOW, HALF_HIGH = 0x3FFFFFFF, 0x40000000  # neighbours whose four bytes all differ: the median sits on a bin's boundary in every round


def named_columns(top: int, seed: int = 11):
    """The columns of the GPU tests over a docID space of `top` documents"""
    d = np.arange(top, dtype=np.uint64)
    r = np.random.default_rng(seed)
    return {"all equal": np.full(top, 0x12345678, dtype=np.uint32), "zeros": np.zeros(top, dtype=np.uint32),
            "ones": np.full(top, M32, dtype=np.uint32), "v = d": d.astype(np.uint32), "reverse": (M32 - d).astype(np.uint32),
            # the top byte ascends with the docID through all 256 digits (v = d << 24, spread over the docID space): the lower bytes equal
            "top byte": (((d * 256 // max(1, top)) << 24) | 0x00C0FFEE).astype(np.uint32),
            "lowest byte": (0x12345600 | ((d * 7) % 251)).astype(np.uint32),
            "two halves": np.where(d % 2 == 0, HALF_LOW, HALF_HIGH).astype(np.uint32),
            "wide": r.integers(0, 1 << 32, top, dtype=np.uint64).astype(np.uint32),
            "half": (d[:top // 2] * 3).astype(np.uint32), "empty": np.zeros(0, dtype=np.uint32)}


def sharing_a_prefix(n: int, first_rank: int):
    """sixteen entries whose ranks among n values are first_rank .. first_rank + 15: on the column v = d, matched whole, values
    that share their three upper bytes where first_rank is a multiple of 256"""
    out = [-(-(first_rank + i) * MILLION // (n - 1)) for i in range(MAX_PERCENTILES)]  # the smallest p with rank_of(n, p) = the rank
    assert [rank_of(n, p) for p in out] == list(range(first_rank, first_rank + MAX_PERCENTILES))
    return out


def percentile_sets(n: int):
    """The sets of the GPU tests; n: the matches of the query that the last set is made for"""
    return {"the minimum": [0], "the maximum": [MILLION], "the median": [500000], "both ends": [0, MILLION],
            "descending, one twice": [999000, 900000, 500000, 500000, 1],
            "sixteen, spread": [i * MILLION // 15 for i in range(MAX_PERCENTILES)],
            "sixteen, one prefix": sharing_a_prefix(n, 4096)}


# ---- the draws of the fuzz cases ----------------------------------------------------------------------------------------
COMMON = (0, 10000, 50000, 100000, 250000, 500000, 750000, 900000, 950000, 990000, 999000, MILLION)


def draw_percentiles(seed: int):
    """One percentile set for a case, from a generator of the case's own: 1 to 16 entries, each with equal chance a common one
    (the ends, the quartiles, the tails) or uniform over 0 .. 1000000, in drawn order — unsorted, repeats possible; every
    third case (seed % 3 == 0) has at least two entries and its first two are 0 and 1000000."""
    r = np.random.default_rng([seed, DRAW_SEED])
    n = int(r.integers(1, MAX_PERCENTILES + 1))
    common = r.random(n) < 0.5
    p = np.where(common, np.array(COMMON)[r.integers(0, len(COMMON), n)], r.integers(0, MILLION + 1, n)).tolist()
    if seed % 3 == 0:
        p = [0, MILLION] + p[2:]
    return [int(x) for x in p]


def conditions(matches, mask, values, per_million, num_docs: int):
    """The fuzz's four conditions of one (case, entry) -> (a short column, some query with more than 256 valued matches — more
    than a page holds, so pages meet in a row —, some query two of whose requested percentiles have different top bytes, some
    query whose requested percentile is a value that more than one of its matches holds); matches: per query every match"""
    many = tops = held = False
    for m in matches:
        s = np.sort(valued(m, mask, values))
        if not s.size:
            continue
        many = many or s.size > 256
        got = [int(s[rank_of(s.size, p)]) for p in per_million]
        tops = tops or len({v >> 24 for v in got}) > 1
        held = held or any(int(np.count_nonzero(s == v)) > 1 for v in got)
    return (len(values) < num_docs, many, tops, held)
