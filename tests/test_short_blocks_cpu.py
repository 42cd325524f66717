"""The short-block cases of tests/short_blocks.py are what they are said to be, and three decoders agree on them: the
encoder's input (the expectation of tests/test_gpu_short_blocks.py) == the C oracle's document_enumerator walk ==
tests/pydecode.py == the instrumented model of every short block's two parts, whose bytes chain to the next block. Then the
floors: every length, every bit width with and without the extra bit on both sides, the code widths, the vbyte sizes, the
(p0, u) pairs, the ticket sizes."""
import numpy as np
import pytest

import oracle
import pydecode
import short_blocks as SB
from dint_amd import host

SINGLE = host.SINGLE_PACKED
PARSE = {host.SINGLE_PACKED: pydecode.parse_single_packed, host.RECTANGULAR: pydecode.parse_rectangular,
         host.MULTI_PACKED: pydecode.parse_multi_packed}


@pytest.mark.parametrize("kind", SB.KINDS)
@pytest.mark.parametrize("which", SB.INDEXES)
def test_the_oracle_and_pydecode_decode_the_encoders_input(which, kind):
    ix = SB.index(which, kind)
    od, of = oracle.OracleDict(kind, ix.docs_dict), oracle.OracleDict(kind, ix.freqs_dict)
    entry_d, entry_f = PARSE[kind](ix.docs_dict), PARSE[kind](ix.freqs_dict)
    same = SB.index(which, SINGLE)
    for i, name in enumerate(ix.names):
        d, f = oracle.posting_list_decode(od, of, ix.index, int(ix.offsets[i]))
        assert np.array_equal(d, ix.lists[i]) and np.array_equal(f, ix.list_freqs[i]), name
        # pydecode: every list of the single-dictionary index; under the other kinds the lists with full blocks, and the
        # short blocks are the single-dictionary index's bytes
        if kind == SINGLE or ix.lens[i] >= 256:
            d, f = pydecode.decode_posting_list(entry_d, entry_f, ix.raw, int(ix.offsets[i]), kind == host.MULTI_PACKED)
            assert np.array_equal(np.array(d, dtype=np.uint32), ix.lists[i]), name
            assert np.array_equal(np.array(f, dtype=np.uint32), ix.list_freqs[i]), name
    for b in np.flatnonzero(ix.blocks["n"] < 256):
        a, e = int(ix.blocks["in_off"][b]), SB.block_end(ix, int(b))
        sa, se = int(same.blocks["in_off"][b]), SB.block_end(same, int(b))
        assert np.array_equal(ix.index[a:e], same.index[sa:se]), (which, int(b))
    if which != "wide":  # (no full block: no dictionary is involved at all)
        assert np.array_equal(ix.index, same.index) and np.array_equal(ix.offsets, same.offsets)


@pytest.mark.parametrize("which", SB.INDEXES)
def test_the_model_of_every_short_block(which):
    """values, the bytes of both parts and their chain, against the encoder's input and pydecode.decode_interpolative"""
    ix = SB.index(which, SINGLE)
    parts = SB.parts(which)
    assert len(parts) == int((ix.blocks["n"] < 256).sum())
    for b, (docs, freqs) in parts.items():
        r = ix.blocks[b]
        n, at, lo = int(r["n"]), int(r["in_off"]), int(r["out_off"])
        want = ix.docids[lo:lo + n].astype(np.int64)
        gaps = np.diff(np.r_[int(r["base"]) - 1, want]) - 1
        assert np.array_equal(docs.values, gaps.astype(np.uint32)) and docs.vbyte == 0
        assert np.array_equal(freqs.values + np.uint32(1), ix.freqs[lo:lo + n])
        assert docs.sum == int(gaps.sum()) and freqs.sum == int(ix.freqs[lo:lo + n].astype(np.int64).sum()) - n
        assert len(docs.widths) == len(freqs.widths) == n - 1
        assert at + docs.size + freqs.size == SB.block_end(ix, b), (which, b)
        g, end = pydecode.decode_interpolative(ix.raw, at, docs.sum, n)
        assert np.array_equal(np.array(g, dtype=np.uint32), docs.values) and end == at + docs.size
        v, end = pydecode.decode_interpolative(ix.raw, end, SB.FREQS_PART, n)
        assert np.array_equal(np.array(v, dtype=np.uint32), freqs.values) and end == at + docs.size + freqs.size
        v, used = oracle.interpolative_decode(ix.index, at + docs.size, SB.FREQS_PART, n)
        assert np.array_equal(v, freqs.values) and used == freqs.size


def test_len_holds_every_length_and_pattern():
    ix = SB.index("len", SINGLE)
    assert ix.lens.tolist() == list(range(1, 256)) and int(ix.docids.max()) < SB.LEN_BOUND
    assert np.array_equal(ix.blocks["n"], ix.lens) and (ix.blocks["base"] == 0).all()
    parts = SB.parts("len")
    for n in range(1, 256):
        docs, freqs = parts[n - 1]
        if n % 5 == 0 or n == 1:
            assert docs.code == 0                                 # all gaps 0, or one posting: no bits
        if n % 5 == 0:
            assert docs.sum == 0 and np.array_equal(ix.lists[n - 1], np.arange(n))
        if n % 5 == 1:
            assert int((docs.values != 0).sum()) == 1 and int(ix.lists[n - 1][-1]) == SB.LEN_BOUND - 1
        if n % 5 == 2:
            assert int(ix.lists[n - 1][0]) == 0 and int(ix.lists[n - 1][-1]) == SB.LEN_BOUND - 1
        if n % 4 == 0:
            assert freqs.sum == 0 and freqs.size == 1             # the vbyte alone
        if n % 4 == 1:
            assert int(freqs.values.max()) >= 1 << 28 and freqs.vbyte == 5
        if n % 4 == 3:
            assert freqs.sum == SB.TOP and freqs.vbyte == 5
    large_at = {int(np.flatnonzero(parts[n - 1][0].values)[0]) * 2 // max(1, n - 1) for n in range(6, 256, 5)}
    assert large_at == {0, 1, 2}                                   # the large gap first, in the middle, last
    one = parts[0]
    assert one[0].size == 0 and one[1].size == one[1].vbyte == 5   # n = 1: no bits at all, the freqs part its vbyte alone


def test_edge_holds_every_pair():
    ix = SB.index("edge", SINGLE)
    parts = SB.parts("edge")
    pairs = SB.edge_pairs()
    assert len(pairs) == 4 * 93 + 4
    want = []
    for k in range(1, 32):
        for u in ((1 << k) - 1, 1 << k, (1 << k) + 1):
            b = u.bit_length() - 1
            m = (1 << (b + 1)) - u
            want += [(which, min(p0, u - 1), u) for which, p0 in enumerate((0, m - 1, m, u - 1))]
    # (93 values of u, 92 of them distinct: 2^1 + 1 = 2^2 - 1)
    assert len(want) == 4 * 93 and want == pairs[:4 * 93] and len({u for _, _, u in want}) == 92
    assert {u for _, _, u in pairs[4 * 93:]} == {(1 << 32) - 1}
    for i, (which, p0, u) in enumerate(pairs):
        docs, freqs = parts[i]  # (a two-posting list is one block: block i is list i)
        b = u.bit_length() - 1
        m = (1 << (b + 1)) - u
        assert freqs.widths == [b] and freqs.extra == [p0 >= m] and int(freqs.values[0]) == p0 and freqs.sum == u - 1
        if u <= SB.TOP:
            assert docs.widths == [b] and docs.extra == [p0 >= m] and ix.lists[i].tolist() == [p0, u]
    assert int(ix.docids.max()) == SB.TOP
    # the extra bit is taken exactly from m on: both sides of it are there for every u that has both
    for u in {u for _, _, u in pairs}:
        mine = {p0 >= ((1 << u.bit_length()) - u) for _, p0, u2 in pairs if u2 == u}
        assert mine == ({False} if u & (u - 1) == 0 else {False, True}), u


def test_wide_tail_and_draws():
    ix = SB.index("wide", SINGLE)
    parts = SB.parts("wide")
    part_of = lambda name: parts[int(ix.blocks_of(name)[-1])]  # noqa: E731
    assert ix.names[-1] == "wide 255" and int(ix.offsets[-1]) == ix.index.size
    for n in SB.WIDE_LENGTHS:
        d = ix.lists[ix.at[f"wide {n}"]]
        assert d.size == n and int(d[0]) == 0 and int(d[-1]) == SB.TOP
    docs, freqs = part_of("wide 255")
    print("wide 255: docs part", docs.size, "bytes, freqs part", freqs.size)
    assert docs.size >= 800 and docs.size == 825 and freqs.sum == SB.TOP
    # TAIL: short blocks behind full ones, base != 0
    for n in SB.TAIL_LENGTHS:
        rows = ix.blocks[ix.blocks_of(f"tail {n}")]
        assert rows["n"].tolist() == [256] * (n // 256) + [n % 256] * (n % 256 != 0)
        assert (rows["base"][1:] != 0).all()
    high = ix.blocks[ix.blocks_of("tail 511")[-1]]
    assert int(high["n"]) == 255 and int(high["base"]) >= 1 << 31 and int(high["max"]) == SB.TOP
    assert int(ix.blocks[ix.blocks_of("tail 257")[-1]]["n"]) == 1
    # the draws
    sizes = [part_of(f"draw {i}")[0].size for i in range(SB.N_DRAWS)]
    print("docs parts of the draws:", sizes)
    assert sum(s > 512 for s in sizes) >= 8 and sum(s < 64 for s in sizes) >= 8
    # a partner shares the chosen half with its list and misses the rest by one
    with_near = 0
    for name, pname in ix.partner_of.items():
        x, p = ix.lists[ix.at[name]].astype(np.int64), ix.lists[ix.at[pname]].astype(np.int64)
        assert np.array_equal(np.intersect1d(x, p), x[::2])
        rest = np.setdiff1d(p, x)
        assert (np.isin(rest - 1, x) | np.isin(rest + 1, x)).all() and rest.size <= x.size // 2
        with_near += int(rest.size != 0)
    assert with_near >= len(ix.partner_of) * 3 // 4


def test_floors():
    seen = {"docs": set(), "freqs": set()}
    lengths, docs_sizes, vbytes = set(), [], set()
    for which in SB.INDEXES:
        ix = SB.index(which, SINGLE)
        for b, (docs, freqs) in SB.parts(which).items():
            lengths.add(int(ix.blocks["n"][b]))
            docs_sizes.append(docs.size)
            vbytes.add(freqs.vbyte)
            seen["docs"] |= set(zip(docs.widths, docs.extra))
            seen["freqs"] |= set(zip(freqs.widths, freqs.extra))
    assert lengths == set(range(1, 256))
    # (width 0 with the extra bit does not exist: read_int(1) reads the value 0 of zero bits, below m = 1)
    want = {(b, False) for b in range(32)} | {(b, True) for b in range(1, 32)}
    assert seen["docs"] == want and seen["freqs"] == want
    assert max(docs_sizes) >= 800 and min(docs_sizes) == 0
    assert {1, 5} <= vbytes


def test_tickets_of_the_cut_tables():
    assert SB.CUT_LENGTHS[:6] == [(255, 4), (201, 5), (165, 6), (141, 7), (121, 8), (107, 9)]
    assert SB.CUT_LENGTHS[-2:] == [(5, 63), (3, 64)]
    tables = SB.cuts(SINGLE)
    assert tuple(tables) == SB.CUT_NAMES
    lanes = {}
    for name, (ix, sh) in tables.items():
        ids, tk = SB.tickets(sh.blocks)
        lanes[name] = [t[1] for t in tk]
        assert sum(lanes[name]) == len(ids) == int((sh.blocks["n"] < 256).sum())
        assert not sh.hole.any() and sh.capacity == int(sh.blocks["n"].sum())
        for first, cnt, row in tk:  # what tails_phase asks of a ticket
            longest = int(sh.blocks["n"][ids[first]])
            assert 1 <= cnt <= 64 and cnt * row <= SB.TICKET_WORDS and row >= longest + 1 + SB.TICKET_STACK and row % 2 == 1
            assert all(int(sh.blocks["n"][b]) <= longest for b in ids[first:first + cnt])
    every = tables["every cut"][1].blocks["n"]
    for n_c, c in SB.CUT_LENGTHS:  # five blocks on both sides of every change
        assert int((every == n_c).sum()) == 5 and (n_c == 255 or int((every == n_c + 1).sum()) == 5)
        assert SB.ticket_lanes(n_c) == c and (n_c == 255 or SB.ticket_lanes(n_c + 1) < c)
    assert 4 in lanes["every cut"] and len(set(lanes["every cut"])) >= 16
    assert lanes["cut 201"] == [4, 4, 2] and lanes["cut 3"] == [10]
    assert lanes["255 then six of 1"] == [4, 3] and lanes["one short block"] == [1] and lanes["no short block"] == []
    assert lanes["two full tickets"] == [64, 64] and lanes["two full tickets and one"] == [64, 64, 1]
    assert len(tables["no short block"][1].blocks) >= 5 and (tables["no short block"][1].blocks["n"] == 256).all()
    all_lanes = {x for v in lanes.values() for x in v}
    assert 4 in all_lanes and 64 in all_lanes
