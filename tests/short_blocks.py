"""The short (binary-interpolative) blocks at their edges (test infrastructure): named posting lists, the indexes built
from them with the product encoder (host.build_index), a plain model of every short block's two parts over
tests/pydecode.py's bit reader, the tickets dint_block_table_create cuts, and block tables built around the ticket cuts.
The expected docIDs and freqs are the encoder's INPUT; tests/test_short_blocks_cpu.py checks that the C oracle and
tests/pydecode.py decode the indexes to it and that the cases are what they are said to be (the floors),
tests/test_gpu_short_blocks.py decodes and queries them on the device.

Three indexes per dictionary kind (a short block's bytes do not depend on the kind; the full blocks of TAIL do):

 len   LEN: one list of every length n = 1 .. 255, docIDs below LEN_BOUND (the ranked calls read norm_lens[docID]).
       Gaps by n % 5: all 0 (no bits: a docs part of 0 bytes) | one large gap at the first, middle or last place | an even
       spread over the range | seeded geometric | 2^j - 1, 2^j, 2^j + 1 in turn. freq - 1 by n % 4: all 0 (a 1-byte vbyte,
       no bits) | one of 2^28 or more (a 5-byte vbyte) | seeded below 2^24 | a sum of exactly 0xFFFFFFFE.
 edge  EDGE: two-posting lists [p0, u]. The block's only node reads p0 in a range of u (read_int(u): b = floor(log2 u) bits,
       one more when the value read is >= m = 2^(b+1) - u): u = 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 31 and p0 = 0, m - 1, m,
       u - 1, clamped to u - 1 (a power of two has m = u: no value takes the extra bit; u = 1 has one value). The freqs part
       of the same list reads the same p0 in the same u (freqs p0 + 1 and u - p0); four more lists carry u = 2^32 - 1 on
       the freqs side. Behind them a partner list for each (below).
 wide  TAIL: lists of 256 + 1, 256 + 255 (the tail's base is 2^31 or more, its max 0xFFFFFFFE), 512 + 128 and 256 postings;
       32 seeded draws (DRAWS); a partner list for each of these and for WIDE; WIDE: 2, 3, 128, 254 and 255 postings spread
       evenly over [0, 0xFFFFFFFE] (255: a docs part of 825 bytes), the list of 255 the last bytes of the index.

A partner list holds every other docID of its list and, for the docIDs between, docID + 1 or docID - 1 where that is no
docID of the list: the AND of the two is the chosen half, the OR counts every near-miss.

The 32 draws: the length uniform in 1 .. 255, the docs range 2^j with j uniform in 0 .. 32, the freqs sum's range likewise,
both capped at 0xFFFFFFFE. Drawn so, far fewer than eight of the 32 have a docs part over 512 bytes (that takes some 200
postings over 2^31: one of the sixteen free draws below has 513): the first eight draw their length from 200 .. 255 and j from 31 .. 32, the next eight j from 0 .. 6, the rest as said.

Width 0 is never read with the extra bit: read_int(1) has b = 0 and m = 1, and the one value it can read is 0. The floors
ask for widths 0 .. 31 without the extra bit and 1 .. 31 with it.
"""
import functools

import numpy as np

import pydecode
import table_shapes as TS
from dint_amd import host

KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]
TOP = 0xFFFFFFFE
LEN_BOUND = 1 << 24
FREQS_PART = 0xFFFFFFFF  # sum_of_values of a freqs part: "a vbyte of the sum comes first"

# dint_block_table_create's tickets (dint_amd/csrc/hip/host/hip_api_index.inc, kernels/index.inc)
TICKET_WORDS, TICKET_STACK, WAVE = 1072, 11, 64


# ---------------------------------------------------------------------------------------------------------------
# the named lists
# ---------------------------------------------------------------------------------------------------------------
def _docids(gaps):
    g = np.asarray(gaps, dtype=np.int64)
    d = np.cumsum(g) + np.arange(g.size)
    assert g.min() >= 0 and int(d[-1]) <= TOP
    return d.astype(np.uint32)


def _freqs(minus_one):
    v = np.asarray(minus_one, dtype=np.int64)
    assert v.min() >= 0 and int(v.sum()) <= TOP  # (a short block stores the sum of freq - 1 as a u32 below 2^32 - 1)
    return (v + 1).astype(np.uint32)


_POW_GAPS = np.array([(1 << j) + d for j in range(1, 18) for d in (-1, 0, 1)], dtype=np.int64)


def len_list(n):
    """-> (docIDs, freqs) of LEN's list of n postings"""
    r = np.random.default_rng(1000 + n)
    room = LEN_BOUND - n  # the gaps may sum to this
    gaps = np.zeros(n, dtype=np.int64)
    if n % 5 == 1:
        gaps[(0, n // 2, n - 1)[(n // 5) % 3]] = room
    elif n % 5 == 2:
        gaps = np.diff(np.r_[-1, (np.arange(n, dtype=np.int64) * (LEN_BOUND - 1)) // (n - 1)]) - 1
    elif n % 5 == 3:
        gaps = r.geometric(1 / 300.0, n).astype(np.int64) - 1
    elif n % 5 == 4:
        gaps = _POW_GAPS[(np.arange(n) + n) % _POW_GAPS.size]
    assert int(gaps.sum()) <= room
    v = np.zeros(n, dtype=np.int64)
    if n % 4 == 1:
        v = r.integers(0, 50, n)
        v[int(r.integers(0, n))] = (1 << 28) + int(r.integers(0, 1 << 28))
    elif n % 4 == 2:
        v = r.integers(0, 1 << 24, n)
    elif n % 4 == 3:
        v = r.integers(0, 1 << 20, n)
        v[int(r.integers(0, n))] += TOP - int(v.sum())
    return _docids(gaps), _freqs(v)


def edge_pairs():
    """-> [(which, p0, u)]: which = 0 .. 3 for p0 = 0, m - 1, m, u - 1 (clamped to u - 1); 4 x 93 of them, then the four of
    u = 2^32 - 1 (freqs side only)"""
    out = []
    us = [(1 << k) + d for k in range(1, 32) for d in (-1, 0, 1)] + [(1 << 32) - 1]
    for u in us:
        b = u.bit_length() - 1
        m = (1 << (b + 1)) - u
        for which, p0 in enumerate((0, m - 1, m, u - 1)):
            out.append((which, min(max(p0, 0), u - 1), u))
    return out


def edge_lists():
    """-> [(docIDs, freqs)], a list per edge_pairs() entry"""
    out = []
    for which, p0, u in edge_pairs():
        if u <= TOP:
            d = np.array([p0, u], dtype=np.uint32)                 # the root reads gap 0 = p0 in [0, max - 1] : u values
        else:
            d = np.array([which, TOP], dtype=np.uint32)
        out.append((d, np.array([p0 + 1, u - p0], dtype=np.uint64).astype(np.uint32)))  # freq - 1 = p0, u - 1 - p0
    return out


def _spread(n, lo=0, hi=TOP):
    return (lo + (np.arange(n, dtype=np.uint64) * np.uint64(hi - lo)) // np.uint64(max(1, n - 1))).astype(np.uint32)


WIDE_LENGTHS = (2, 3, 128, 254, 255)


def wide_list(n):
    r = np.random.default_rng(2000 + n)
    v = np.sort(r.integers(0, TOP + 1, n - 1))
    return _spread(n), _freqs(np.diff(np.r_[0, v, TOP]))  # freq - 1: n values summing to 0xFFFFFFFE, spread like the docIDs


TAIL_LENGTHS = (256 + 1, 256 + 255, 512 + 128, 256)


def tail_list(n):
    r = np.random.default_rng(3000 + n)
    gaps = r.geometric(0.05, n).astype(np.int64) - 1
    d = np.cumsum(gaps) + np.arange(n)
    f = r.geometric(0.5, n).astype(np.int64)
    if n == 256 + 255:  # full block up to 2^31 and a little, the tail spread from there to 0xFFFFFFFE
        d[:256] += (1 << 31) - int(d[200])
        d[256:] = _spread(255, int(d[255]) + 1 + 12345, TOP)
        f[256:] = _freqs(r.integers(0, 1 << 24, 255))
    else:
        d += 1000 * n
    return d.astype(np.uint32), f.astype(np.uint32)


N_DRAWS = 32


def draw_list(i):
    r = np.random.default_rng(4000 + i)
    n = int(r.integers(1, 256))
    j, jf = int(r.integers(0, 33)), int(r.integers(0, 33))
    if i < 8:
        n, j = int(r.integers(200, 256)), int(r.integers(31, 33))
    elif i < 16:
        j = int(r.integers(0, 7))
    total = min(1 << j, TOP - (n - 1))
    ftotal = min(1 << jf, TOP)
    gaps = np.diff(np.r_[0, np.sort(r.integers(0, total + 1, n))])
    v = np.diff(np.r_[0, np.sort(r.integers(0, ftotal + 1, n))])
    return _docids(gaps), _freqs(v)


def partner(docids, seed):
    """-> (docIDs, freqs): every other docID of the list, and next to the ones between a docID the list does not hold"""
    r = np.random.default_rng(5000 + seed)
    x = np.asarray(docids, dtype=np.int64)
    between = x[1::2]
    near = between + np.where(np.arange(between.size) % 2 == 0, 1, -1)
    near = np.setdiff1d(near[(near >= 0) & (near <= TOP)], x)
    p = np.union1d(x[::2], near)
    return p.astype(np.uint32), r.integers(1, 1000, p.size).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------
# the indexes
# ---------------------------------------------------------------------------------------------------------------
class Index:
    """names[i] / lists[i] / list_freqs[i]: the lists as given to the encoder; docids / freqs: back to back, list i =
    [bounds[i], bounds[i + 1]); index / offsets: host.build_index's; blocks: the block table read from the lists'
    directories (table_shapes.block_table: what dint_index_posting_lists returns); partner_of: {list: its partner}."""

    def __init__(self, kind, named, partner_of=None):
        self.kind = kind
        self.names = [x[0] for x in named]
        self.at = {name: i for i, name in enumerate(self.names)}
        assert len(self.at) == len(self.names)
        self.lists = [np.asarray(x[1], dtype=np.uint32) for x in named]
        self.list_freqs = [np.asarray(x[2], dtype=np.uint32) for x in named]
        self.partner_of = partner_of or {}
        self.lens = np.array([x.size for x in self.lists], dtype=np.uint32)
        self.docids = np.concatenate(self.lists)
        self.freqs = np.concatenate(self.list_freqs)
        self.bounds = np.concatenate([[0], np.cumsum(self.lens.astype(np.int64))])
        for x in self.lists:
            assert x.size and np.all(np.diff(x.astype(np.int64)) > 0)
        gaps = np.concatenate([host.docids_to_gaps(x) for x in self.lists])
        self.docs_dict = host.build_dictionary(kind, host.Collection(gaps, self.lens))
        self.freqs_dict = host.build_dictionary(kind, host.Collection(self.freqs - np.uint32(1), self.lens))
        self.index, self.offsets = host.build_index(kind, self.docs_dict, self.freqs_dict, self.docids, self.freqs, self.lens)
        self.raw = self.index.tobytes()  # (for tests/pydecode.py: plain Python integers)
        self.blocks = TS.block_table(self)
        assert np.array_equal(self.blocks["max"], self.docids[(self.blocks["out_off"] + self.blocks["n"] - 1).astype(np.int64)])

    bytes = property(lambda self: self.index)

    def blocks_of(self, name):
        return np.flatnonzero(self.blocks["list"] == self.at[name])


def _with_partners(named, first_seed):
    partners, of = [], {}
    for k, (name, d, _f) in enumerate(named):
        partners.append(("partner of " + name, *partner(d, first_seed + k)))
        of[name] = partners[-1][0]
    return partners, of


def len_named():
    return [(f"len {n}", *len_list(n)) for n in range(1, 256)]


def edge_named():
    return [(f"edge {i} which={w} p0={p0} u={u}", d, f) for i, ((w, p0, u), (d, f)) in enumerate(zip(edge_pairs(), edge_lists()))]


def wide_named():
    tails = [(f"tail {n}", *tail_list(n)) for n in TAIL_LENGTHS]
    draws = [(f"draw {i}", *draw_list(i)) for i in range(N_DRAWS)]
    wide = [(f"wide {n}", *wide_list(n)) for n in WIDE_LENGTHS]
    return tails, draws, wide


@functools.lru_cache(maxsize=None)
def index(which, kind):
    """which: "len", "edge" or "wide\""""
    if which == "len":
        return Index(kind, len_named())
    if which == "edge":
        named = edge_named()
        partners, of = _with_partners(named, 0)
        return Index(kind, named + partners, of)
    tails, draws, wide = wide_named()
    partners, of = _with_partners(tails + draws + wide, 1000)
    return Index(kind, tails + draws + partners + wide, of)  # (the list of 255 over the whole range: the index's last bytes)


INDEXES = ("len", "edge", "wide")


# ---------------------------------------------------------------------------------------------------------------
# the model of a short block: tests/pydecode.py's reader, instrumented
# ---------------------------------------------------------------------------------------------------------------
class _Probe(pydecode._Bits):
    """pydecode's bit reader, noting of every read_int the width b and whether the value took the extra bit"""

    def __init__(self, data, pos):
        super().__init__(data, pos)
        self.widths, self.extra = [], []

    def read_int(self, u):
        before = self.bit
        v = super().read_int(u)
        b = u.bit_length() - 1
        assert self.bit - before in (b, b + 1)
        self.widths.append(b)
        self.extra.append(self.bit - before == b + 1)
        return v


class Part:
    """One part of a short block: values (the gaps, or freq - 1), widths / extra per value read, vbyte: the bytes of the
    leading sum (0: a docs part), code: the bytes of the interpolative code, size = vbyte + code, sum: the sum of values."""

    def __init__(self, values, widths, extra, vbyte, code, total):
        self.values, self.widths, self.extra, self.vbyte, self.code, self.sum = values, widths, extra, vbyte, code, total
        self.size = vbyte + code


def probe_part(data, pos, sum_of_values, n):
    """interpolative_block::decode as pydecode.decode_interpolative does it, through the instrumented reader"""
    start = pos
    if sum_of_values == FREQS_PART:
        sum_of_values, shift = 0, 0
        while True:
            c = int(data[pos])
            pos += 1
            sum_of_values += (c & 127) << shift
            shift += 7
            if c & 128:
                break
    out = [0] * n
    out[n - 1] = sum_of_values
    bits = _Probe(data, pos)
    if n > 1:
        pydecode._interp(bits, out, 0, n - 1, 0, sum_of_values)
    values = np.diff(np.r_[0, np.array(out, dtype=np.int64)]).astype(np.uint32)
    return Part(values, bits.widths, bits.extra, pos - start, (bits.bit + 7) // 8, sum_of_values)


def block_parts(ix, b):
    """Block b (fewer than 256 postings) of ix.blocks -> (docs Part, freqs Part)"""
    r = ix.blocks[b]
    n, at = int(r["n"]), int(r["in_off"])
    assert n < 256
    docs = probe_part(ix.raw, at, int(r["max"]) - int(r["base"]) - (n - 1), n)
    return docs, probe_part(ix.raw, at + docs.size, FREQS_PART, n)


@functools.lru_cache(maxsize=None)
def parts(which, kind=host.SINGLE_PACKED):
    """{block: (docs Part, freqs Part)} of every short block of index(which, kind). (The parts of a short block are the
    same bytes under every kind — test_short_blocks_cpu.py — so the single-dictionary index's serve all three.)"""
    ix = index(which, kind)
    return {int(b): block_parts(ix, int(b)) for b in np.flatnonzero(ix.blocks["n"] < 256)}


def block_end(ix, b):
    """Where block b's bytes end: the next block of its list, or the next list"""
    if b + 1 < len(ix.blocks) and ix.blocks["list"][b + 1] == ix.blocks["list"][b]:
        return int(ix.blocks["in_off"][b + 1])
    return int(ix.offsets[int(ix.blocks["list"][b]) + 1])


# ---------------------------------------------------------------------------------------------------------------
# tickets and the tables around their cuts
# ---------------------------------------------------------------------------------------------------------------
def ticket_lanes(n):
    """Lanes of a ticket whose longest block has n postings"""
    row = (n + 1 + TICKET_STACK) | 1
    return min(WAVE, TICKET_WORDS // row)


def tickets(blocks):
    """dint_block_table_create's schedule of a table's short blocks: sorted longest first (stable), cut into tickets of
    as many blocks as fit a wave's scratch at the row of the ticket's longest -> (ids, [(first, lanes, row words)])"""
    n = blocks["n"]
    ids = sorted(np.flatnonzero(n < 256).tolist(), key=lambda b: -int(n[b]))
    out, i = [], 0
    while i < len(ids):
        row = (int(n[ids[i]]) + 1 + TICKET_STACK) | 1
        lanes = min(WAVE, TICKET_WORDS // row, len(ids) - i)
        out.append((i, lanes, row))
        i += lanes
    return ids, out


#: (longest block of a ticket of that many lanes, lanes): 255/4, 201/5, 165/6, 141/7, 121/8, 107/9, ... 5/63, 3/64
CUT_LENGTHS = [(max(n for n in range(1, 256) if ticket_lanes(n) == c), c) for c in range(4, 65)
               if any(ticket_lanes(n) == c for n in range(1, 256))]

CUT_NAMES = ("every cut", "cut 201", "cut 107", "cut 5", "cut 3", "255 then six of 1", "one short block", "no short block",
             "two full tickets", "two full tickets and one")


def cuts(kind):
    """Block tables around the ticket cuts -> {name: (Index, table_shapes.BlockShape)}: blocks of LEN chosen by length (a
    list of LEN is one block; the same block may stand in several entries, each with an output of its own), outputs back to
    back. `no short block`: TAIL's full blocks.

    A wave draws a second ticket (the `tk += gridDim.x * kWavesPerBlock` loop of tails_phase) only in a table of more
    tickets than 16 x the docs launch's grid, and the grid is min(ceil(blocks / 16), compute units) workgroups
    (decode_grid, hip_api_vroom.inc): up to 4096 blocks there is a wave per block, beyond that 20 000 blocks of up to 3
    postings are 313 tickets for 4096 waves. No such table is here."""
    r = np.random.default_rng(77)
    lx, wx = index("len", kind), index("wide", kind)

    def of_lengths(name, lengths, shuffle=False):
        rows = np.array([n - 1 for n in lengths], dtype=np.int64)  # LEN's list of n postings is block n - 1
        if shuffle:
            rows = r.permutation(rows)
        n = lx.blocks["n"][rows]
        assert sorted(n.tolist()) == sorted(lengths)
        return lx, TS._block_shape(name, lx, lx.blocks, rows, TS._back_to_back(n), int(n.sum()))

    def both_sides(n_c):
        return [n_c + 1] * 5 * (n_c + 1 < 256) + [n_c] * 5

    out = {}
    out["every cut"] = of_lengths("every cut", [n for n_c, _ in CUT_LENGTHS for n in both_sides(n_c)], shuffle=True)
    for n_c in (201, 107, 5, 3):
        out[f"cut {n_c}"] = of_lengths(f"cut {n_c}", both_sides(n_c))
    out["255 then six of 1"] = of_lengths("255 then six of 1", [255] + [1] * 6)
    out["one short block"] = of_lengths("one short block", [131])
    full = np.flatnonzero(wx.blocks["n"] == 256)
    out["no short block"] = (wx, TS._block_shape("no short block", wx, wx.blocks, full, TS._back_to_back(wx.blocks["n"][full]), 256 * full.size))
    small = [1 + k % 3 for k in range(2 * WAVE)]
    out["two full tickets"] = of_lengths("two full tickets", small)
    out["two full tickets and one"] = of_lengths("two full tickets and one", small + [2])
    assert tuple(out) == CUT_NAMES
    return out
