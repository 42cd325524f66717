"""Reshaped unit and block tables over the fuzz cases (test infrastructure).

dint_index_stream, dint_index_posting_lists and the fuzz generator (tests/fuzz_streams.py) all make tables in stream
order, outputs back to back, every list present. The C ABI takes any table (include/dint_hip.h: dint_decode_units,
dint_unit_table_create, dint_block_ref, dint_decode_posting_blocks): this module reorders, subsets, scatters, repeats and
overlaps the entries of a fuzz case's own tables and moves the generator's expected integers to each entry's new place.
No decoder runs here; everything is seeded. tests/test_table_shapes_cpu.py checks the expectations against the C oracle,
tests/test_gpu_table_shapes.py decodes the shapes on the device.

A shape's expectation covers its WHOLE output buffer: `want` holds the integers, `hole` marks what no entry writes (it
must keep whatever the buffer held before the decode)."""
import numpy as np

import fuzz_streams as F

#: dint_block_ref (include/dint_hip.h)
BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("n", "<u4"), ("base", "<u4"), ("max", "<u4"),
                        ("list", "<u4")])

#: the unit shapes (OVERLAP_SHAPES: single-dictionary streams only — a multi unit of at most 256 integers is a whole block)
UNIT_SHAPES = ("permuted", "reversed", "every_other_list", "random_subset", "scattered", "repeated", "mixed")
OVERLAP_SHAPES = ("overlapping",)
BLOCK_SHAPES = ("lists_permuted", "lists_subset", "blocks_reversed", "blocks_permuted", "blocks_repeated",
                "blocks_scattered", "short_only", "full_only")


class UnitShape:
    """units: UNIT_DTYPE[]; want / hole: the output buffer (u32[capacity] / bool[capacity]); ends: u64 per unit;
    src: where each unit's integers start in the case's expected output (FuzzStream.expect)."""

    def __init__(self, name, units, want, hole, ends, src):
        self.name, self.units, self.want, self.hole, self.ends, self.src = name, units, want, hole, ends, src

    @property
    def capacity(self):
        return len(self.want)


class BlockShape:
    """blocks: BLOCK_DTYPE[]; docids / freqs / hole: the two output buffers (u32[capacity] each) and what stays
    untouched; src: where each block's postings start in FuzzIndex.docids / freqs."""

    def __init__(self, name, blocks, docids, freqs, hole, src):
        self.name, self.blocks, self.docids, self.freqs, self.hole, self.src = name, blocks, docids, freqs, hole, src

    @property
    def capacity(self):
        return len(self.docids)


# ---------------------------------------------------------------------------------------------------------------
# placing entries in an output buffer
# ---------------------------------------------------------------------------------------------------------------
def _back_to_back(n, start=0):
    n = np.asarray(n, dtype=np.int64)
    return start + np.cumsum(n) - n


def _scatter(r, n, zero_p=0.3):
    """Every entry at a random place, a hole of 1 to 300 integers in front of it (none, with probability zero_p: those
    entries follow an output that is not their table neighbour's) -> (out offsets, capacity)"""
    n = np.asarray(n, dtype=np.int64)
    order = r.permutation(len(n))
    gaps = np.where(r.random(len(n)) < zero_p, 0, r.integers(1, 301, len(n)))
    placed = np.cumsum(gaps + n[order]) - n[order]
    outs = np.empty(len(n), dtype=np.int64)
    outs[order] = placed
    return outs, int(placed[-1] + n[order[-1]] + r.integers(1, 301)) if len(n) else 0


def _spread(n, dst, src):
    """Index arrays (into the output, into the source) of every integer of entries (n, dst, src)."""
    n = np.asarray(n, dtype=np.int64)
    total = int(n.sum())
    within = np.arange(total) - np.repeat(np.cumsum(n) - n, n)
    return np.repeat(np.asarray(dst, dtype=np.int64), n) + within, np.repeat(np.asarray(src, dtype=np.int64), n) + within


def _fill(sources, n, outs, srcs, capacity):
    """-> ([u32[capacity] per source], hole mask); entries must not share an output integer."""
    di, si = _spread(n, outs, srcs)
    hole = np.ones(capacity, dtype=bool)
    hole[di] = False
    assert capacity - hole.sum() == di.size, "two entries write the same output integer"
    filled = []
    for s in sources:
        w = np.zeros(capacity, dtype=np.uint32)
        w[di] = s[si]
        filled.append(w)
    return filled, hole


# ---------------------------------------------------------------------------------------------------------------
# unit tables
# ---------------------------------------------------------------------------------------------------------------
def whole_lists(S):
    """One unit per list, as dint_index_stream(enc, 0) cuts a stream of lists below DINT_MAX_UNIT_INTS -> (units, ends)"""
    units = np.array([(off, first, n, li) for li, (off, n, first) in enumerate(S.lists)], dtype=F.UNIT_DTYPE)
    last = np.r_[S.units["list"][1:] != S.units["list"][:-1], True]
    assert np.array_equal(S.units["list"][last], np.arange(len(S.lists)))
    return units, S.ends[last].astype(np.uint64)


def cut_ends(S, units):
    """End offsets of a complete stream-order cut of S's lists (the generator's, or dint_index_stream's): a unit ends where
    the next unit of its list starts, the last one where the list ends."""
    _, list_end = whole_lists(S)
    ends = list_end[units["list"]].copy()
    same = units["list"][1:] == units["list"][:-1]
    ends[:-1][same] = units["in_off"][1:][same]
    return ends


def _unit_shape(name, S, pool, pool_ends, rows, outs, capacity):
    rows = np.asarray(rows, dtype=np.int64)
    units = pool[rows].copy()
    src = pool["out_off"][rows].astype(np.int64)
    units["out_off"] = np.asarray(outs, dtype=np.uint64)
    (want,), hole = _fill([S.expect], units["n"], units["out_off"], src, capacity)
    return UnitShape(name, units, want, hole, pool_ends[rows].astype(np.uint64), src)


def overlap_groups(S, units, ends):
    """Lists of at most 256 integers that `units` (a complete stream-order cut) cuts in two or more: -> [(list, rows)]"""
    out = []
    starts = np.flatnonzero(np.r_[True, units["list"][1:] != units["list"][:-1]])
    stops = np.r_[starts[1:], len(units)]
    for a, b in zip(starts, stops):
        li = int(units["list"][a])
        if b - a >= 2 and S.lists[li][1] <= 256:
            out.append((li, np.arange(a, b)))
    return out


def unit_shapes(S, kind, seed, cuts=()):
    """The reshaped unit tables of a fuzz stream -> {name: UnitShape}.
    cuts: more complete stream-order cuts of the same stream (dint_index_stream(enc, 256), (enc, 77), ...): the mixed shape
    takes its pieces from the first (single-dictionary streams; else from the generator's units), the overlapping shape
    its pairs from all of them and from the generator's."""
    r = np.random.default_rng(seed)
    own, own_ends = S.units, S.ends
    whole, whole_ends = whole_lists(S)
    m, total = len(own), len(S.expect)
    shapes = {}

    perm = r.permutation(m)
    shapes["permuted"] = _unit_shape("permuted", S, own, own_ends, perm, own["out_off"][perm], total)
    rev = np.arange(m)[::-1]
    shapes["reversed"] = _unit_shape("reversed", S, own, own_ends, rev, own["out_off"][rev], total)
    # subsets, outputs compacted: the table skips stream bytes (a span taken from the next entry overestimates the unit)
    for name, rows in (("every_other_list", np.flatnonzero(own["list"] % 2 == 0)),
                       ("random_subset", np.sort(r.choice(m, max(2, int(0.3 * m)), replace=False)))):
        n = own["n"][rows]
        shapes[name] = _unit_shape(name, S, own, own_ends, rows, _back_to_back(n), int(n.sum()))
    outs, cap = _scatter(r, own["n"])
    shapes["scattered"] = _unit_shape("scattered", S, own, own_ends, np.arange(m), outs, cap)
    # every unit twice, the copy right behind it in the table and in the output: two entries with one in_off
    rows = np.repeat(np.arange(m), 2)
    shapes["repeated"] = _unit_shape("repeated", S, own, own_ends, rows, _back_to_back(own["n"][rows]), 2 * total)
    # whole lists beside lists in pieces, one table (stream order, every integer at its own place)
    pieces, piece_ends = (cuts[0], cut_ends(S, cuts[0])) if cuts and kind != F.MULTI else (own, own_ends)
    as_whole = r.random(len(S.lists)) < 0.5
    pool = np.concatenate([whole[as_whole], pieces[~as_whole[pieces["list"]]]])
    pool_ends = np.concatenate([whole_ends[as_whole], piece_ends[~as_whole[pieces["list"]]]])
    order = np.lexsort((pool["in_off"], pool["list"]))
    shapes["mixed"] = _unit_shape("mixed", S, pool[order], pool_ends[order], np.arange(len(pool)), pool[order]["out_off"], total)
    if kind != F.MULTI:
        # a whole list of at most 256 integers, then its later pieces, outputs back to back (one bundle): the next entry of
        # the table starts INSIDE the first unit's bytes
        rows_w, rows_p, tables = [], [], []
        for t, (u, e) in enumerate([(own, own_ends)] + [(c, cut_ends(S, c)) for c in cuts]):
            tables.append((u, e))
            for li, rows in overlap_groups(S, u, e):
                rows_w.append(li)
                rows_p.append((t, rows[1:]))
        pool = np.concatenate([whole] + [u for u, _ in tables])
        pool_ends = np.concatenate([whole_ends] + [e for _, e in tables])
        base = np.cumsum([len(whole)] + [len(u) for u, _ in tables])
        rows = []
        for li, (t, p) in zip(rows_w, rows_p):
            rows += [li] + list(base[t] + p)
        n = pool["n"][rows]
        shapes["overlapping"] = _unit_shape("overlapping", S, pool, pool_ends, rows, _back_to_back(n), int(n.sum()))
    return shapes


def cut_into(shape):
    """Entries that a LATER table entry begins strictly inside of (by their true byte spans: in_off .. ends): the one table
    dint_decode_units does not promise to decode right (include/dint_hip.h) -> bool per entry"""
    import bisect

    u = shape.units
    out = np.zeros(len(u), dtype=bool)
    later = []
    for i in range(len(u) - 1, -1, -1):
        a = int(u["in_off"][i])
        k = bisect.bisect_right(later, a)
        out[i] = k < len(later) and later[k] < int(shape.ends[i])
        bisect.insort(later, a)
    return out


def overlap_pairs(shape):
    """The (whole list, first later piece) pairs of an overlapping shape: table rows i, i + 1."""
    u = shape.units
    i = np.flatnonzero((u["list"][1:] == u["list"][:-1]) & (u["in_off"][1:] > u["in_off"][:-1]) &
                       (u["out_off"][1:] == u["out_off"][:-1] + u["n"][:-1]) & (u["in_off"][1:] < shape.ends[:-1]))
    return i[(u["n"][i] <= 256)]


# ---------------------------------------------------------------------------------------------------------------
# block tables
# ---------------------------------------------------------------------------------------------------------------
def _vbyte_read(buf, at):
    v, shift = 0, 0
    while True:
        b = int(buf[at])
        at += 1
        v |= (b & 127) << shift
        if b & 128:
            return v, at
        shift += 7


def block_table(X):
    """dint_index_posting_lists over a fuzz index, read from the dict_posting_list layout
    (vbyte(n) | u32 max[B] | u32 endpoint[B-1] | blocks) -> BLOCK_DTYPE[] (lists in order, outputs back to back)"""
    rows = []
    for li in range(len(X.offsets) - 1):
        n, at = _vbyte_read(X.index, int(X.offsets[li]))
        nb = (n + 255) // 256
        maxs = np.frombuffer(X.index[at: at + 4 * nb].tobytes(), dtype="<u4")
        ends = np.frombuffer(X.index[at + 4 * nb: at + 8 * nb - 4].tobytes(), dtype="<u4")
        body = at + 8 * nb - 4
        for b in range(nb):
            rows.append((body + (int(ends[b - 1]) if b else 0), int(X.bounds[li]) + 256 * b, min(256, n - 256 * b),
                         int(maxs[b - 1]) + 1 if b else 0, int(maxs[b]), li))
    return np.array(rows, dtype=BLOCK_DTYPE)


def _block_shape(name, X, blocks, rows, outs, capacity):
    rows = np.asarray(rows, dtype=np.int64)
    t = blocks[rows].copy()
    src = blocks["out_off"][rows].astype(np.int64)
    t["out_off"] = np.asarray(outs, dtype=np.uint64)
    (docids, freqs), hole = _fill([X.docids, X.freqs], t["n"], t["out_off"], src, capacity)
    return BlockShape(name, t, docids, freqs, hole, src)


def block_shapes(X, blocks, seed):
    """The reshaped block tables of a fuzz index (blocks: its table, block_table(X) or dint_index_posting_lists') ->
    {name: BlockShape}. Every ref keeps its base and max."""
    r = np.random.default_rng(seed)
    nb, total = len(blocks), int(blocks["n"].sum())
    n_lists = int(blocks["list"].max()) + 1
    by_list = [np.flatnonzero(blocks["list"] == li) for li in range(n_lists)]
    shapes = {}

    def compact(name, rows):
        n = blocks["n"][rows]
        shapes[name] = _block_shape(name, X, blocks, rows, _back_to_back(n), int(n.sum()))

    compact("lists_permuted", np.concatenate([by_list[li] for li in r.permutation(n_lists)]))
    keep = np.sort(r.choice(n_lists, max(2, int(0.3 * n_lists)), replace=False))
    compact("lists_subset", np.concatenate([by_list[li] for li in keep]))
    rev = np.arange(nb)[::-1]
    shapes["blocks_reversed"] = _block_shape("blocks_reversed", X, blocks, rev, blocks["out_off"][rev], total)
    perm = r.permutation(nb)
    shapes["blocks_permuted"] = _block_shape("blocks_permuted", X, blocks, perm, blocks["out_off"][perm], total)
    rows = np.repeat(np.arange(nb), 2)
    outs = blocks["out_off"][rows].astype(np.int64) + np.tile([0, total], nb)
    shapes["blocks_repeated"] = _block_shape("blocks_repeated", X, blocks, rows, outs, 2 * total)
    outs, cap = _scatter(r, blocks["n"])
    shapes["blocks_scattered"] = _block_shape("blocks_scattered", X, blocks, np.arange(nb), outs, cap)
    compact("short_only", np.flatnonzero(blocks["n"] < 256))
    compact("full_only", np.flatnonzero(blocks["n"] == 256))
    return shapes
