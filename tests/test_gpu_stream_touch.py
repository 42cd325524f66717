"""The vroom single-dictionary segments touch the rest of their unit's stream in the prologue's trip to memory (kernels/segment.inc,
TOUCH; the window rule: dint_stream_touch.hpp, pinned case by case in tests/test_stream_touch_cpu.py): one dword a lane at a
128-byte stride from the line of tile 3's first byte on, up to 64 lanes by the unit's n, clipped at the stream's end. Its value is
used for nothing, so what can go wrong is an address: these are the smallest shapes at which the window meets the end of the
buffer, the next unit, units already decoded, and offset 2^32. Streams are assembled slot by slot as in
tests/test_gpu_stream_bursts.py (whose pieces this file uses), every one decoded through dint_decode_units and through a prepared
UnitTable, integers and end offsets bit for bit against the assembler's input, canary words behind every unit's output, the
device copy of a stream exactly as long as the stream. No test looks for a fault: the bounds are the CPU cases'.

A unit is touched ahead when its n is above 2588 (n * 19 / 32 bytes expected, 1536 of them the prologue's own): units of `big`
codewords reach that in a tile or two and their windows run far past their own bytes, units of `small` codewords span the
9 KB and more that the rule expects of them."""
import numpy as np
import pytest

import fuzz_streams as F
import test_gpu_stream_bursts as SB

pytestmark = pytest.mark.gpu

TILE = SB.TILE
TOUCH_N = 2589  # the smallest n with a window


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev  # fails loudly if libdint_hip.so is missing

    return dev


@pytest.fixture(scope="module")
def fuzz_dict():
    D = F.make_dictionary(np.random.default_rng(77001), F.SINGLE, m_entries=65536, value_profile="mixed", size_profile="pow2")
    assert {1, 2, 4, 16} <= set(D.by_size[0])
    return D


@pytest.fixture(scope="module")
def dictionary(device, fuzz_dict):
    return device.Dictionary(fuzz_dict.kind, fuzz_dict.file)


def sized(r, D, n_slots, sizes):
    """n_slots one-slot codewords of the given sizes (integers a codeword decodes to)."""
    pool = np.concatenate([D.by_size[0][s] for s in sizes])
    return r.choice(pool, n_slots).astype(np.int64), np.zeros(n_slots, dtype=np.int64)


def ints(r, D, n, sizes=None, exc_p=0.02):
    """Codewords that decode to EXACTLY n integers: any id (runs included) or ids of the given sizes, some exceptions, one-integer
    codewords at the end."""
    ids, lits, have = [], [], 0
    pool = None if sizes is None else np.concatenate([D.by_size[0][s] for s in sizes])
    while have < n:
        if n - have < 256:
            i, lit = int(r.choice(D.by_size[0][1])), 0
        elif r.random() < exc_p:
            i = int(r.integers(0, 2))
            lit = int(r.integers(0, 1 << (16 if i == 0 else 32)))
        else:
            i, lit = int(r.integers(2, len(D.size[0])) if pool is None else r.choice(pool)), 0
        ids.append(i)
        lits.append(lit)
        have += int(D.size[0][i])
    assert have == n
    return np.array(ids, dtype=np.int64), np.array(lits, dtype=np.int64)


def n_of(D, part):
    return int(D.size[0][part[0]].sum())


def test_units_of_one_to_four_tiles(device, dictionary, fuzz_dict):
    """256 k - 1, 256 k and 256 k + 1 slots, k = 1..4, of codewords of 16 integers (n from 4080 on: every one has a window, all of it
    in the units that follow or past the stream's end) and of codewords of 1 and 2 (n below the threshold: none has)."""
    r = np.random.default_rng(11)
    parts, residues = [], []
    for j, s in enumerate(TILE * k + e for k in range(1, 5) for e in (-1, 0, 1)):
        parts += [sized(r, fuzz_dict, s, (16,)), sized(r, fuzz_dict, s, (1, 2)), SB.craft(r, fuzz_dict, s)]
        residues += [(41 * j) % 128, (41 * j + 64) % 128, 127 - j]
    assert min(n_of(fuzz_dict, p) for p in parts[0::3]) >= TOUCH_N > max(n_of(fuzz_dict, p) for p in parts[1::3])
    SB.check(device, dictionary, SB.assemble(fuzz_dict, parts, residues, tail_pad=3))


@pytest.mark.parametrize("sizes", [None, (1, 2, 4)], ids=["big", "small"])
@pytest.mark.parametrize("lead", [0, 1, 127])
def test_a_unit_of_16384_integers_that_ends_with_the_buffer(device, dictionary, fuzz_dict, sizes, lead):
    """The full window of 64 lanes: inside the unit (`small`: 14 KB of stream) or reaching past it (`big`: 5 KB) — past the buffer's
    last byte, that is; then the same unit with a unit of one integer behind it, whose two bytes are the stream's last."""
    r = np.random.default_rng(21 + lead)
    unit = ints(r, fuzz_dict, 16384, sizes)
    B = SB.assemble(fuzz_dict, [unit], residues=[lead])
    assert int(B.units["n"][0]) == 16384 and int(B.ends[-1]) == B.enc.size and (sizes is None) == (B.enc.size < 9216)
    SB.check(device, dictionary, B)
    B = SB.assemble(fuzz_dict, [unit, ints(r, fuzz_dict, 1)], residues=[lead, B.enc.size % 128])
    assert list(B.units["n"]) == [16384, 1] and int(B.ends[-1]) == B.enc.size and int(B.units["in_off"][1]) == B.enc.size - 2
    SB.check(device, dictionary, B)


@pytest.mark.parametrize("last_slots,last_sizes", [(700, (16,)), (767, (16,)), (769, (16,)), (2500, (4, 16)), (6000, (1, 2, 4))],
                         ids=["1400B", "1534B", "1538B", "5000B", "12000B"])
def test_the_last_unit_begins_near_the_streams_end(device, dictionary, fuzz_dict, last_slots, last_sizes):
    """The last unit of a table begins less than 1.5 KB before the stream's end (tile 3 would begin past it: no window, for all
    its n of 11200), just past 1.5 KB (a window of one line), less than 8 KB (the window is cut at the end) and more than 8 KB
    before it (the whole window fits); a unit of 16384 integers in front of it, whose window covers the last unit's bytes."""
    r = np.random.default_rng(last_slots)
    parts = [ints(r, fuzz_dict, 16384), sized(r, fuzz_dict, last_slots, last_sizes)]
    assert n_of(fuzz_dict, parts[1]) >= TOUCH_N
    B = SB.assemble(fuzz_dict, parts, residues=[3, 101])
    assert B.enc.size - int(B.units["in_off"][-1]) == 2 * last_slots
    SB.check(device, dictionary, B)


def test_a_unit_table_visited_in_reverse(device, dictionary, fuzz_dict):
    """The table's first unit is the stream's last: what a unit touches ahead belongs to units already decoded (or being decoded by
    another wave); more units than a workgroup has waves."""
    r = np.random.default_rng(31)
    ns = [16384, 3000, 9000, 2589, 16384, 2588, 5000, 12000] * 3
    parts = [ints(r, fuzz_dict, n, (1, 2, 4) if j % 2 else None) for j, n in enumerate(ns)]
    B = SB.assemble(fuzz_dict, parts, residues=[(53 * j) % 128 for j in range(len(ns))])
    assert list(B.units["n"]) == ns
    B.units, B.ends = B.units[::-1].copy(), B.ends[::-1].copy()
    assert np.all(np.diff(B.units["in_off"].astype(np.int64)) < 0)
    SB.check(device, dictionary, B)


@pytest.mark.parametrize("cut", [1536 + 77, 4099, 20000])
def test_a_stream_placed_across_4_gib(device, dictionary, fuzz_dict, cut):
    """As tests/test_gpu_parity.py places its corpus (test_a_stream_that_straddles_4_gib): the stream's byte `cut` at offset 2^32 of a
    4.3 GB buffer that ends with the stream — 2^32 falls inside the first unit's window (its tile 3 a line below it), inside a
    later pair of it, and inside a later unit. The arithmetic on in_off, the window's first line and the room left is 64-bit."""
    import torch

    r = np.random.default_rng(cut)
    parts = [ints(r, fuzz_dict, 16384, (1, 2, 4)), ints(r, fuzz_dict, 16384), ints(r, fuzz_dict, 4000, (1, 2, 4)), ints(r, fuzz_dict, 16384)]
    B = SB.assemble(fuzz_dict, parts, residues=[0, 19, 64, 127])
    assert int(B.ends[0]) > 12000 and int(B.ends[0]) < 20000 < int(B.ends[1]) and B.enc.size > cut
    dev = torch.device("cuda", 0)
    shift = (1 << 32) - cut
    big = torch.zeros(shift + B.enc.size, dtype=torch.uint8, device=dev)
    big[shift:] = torch.from_numpy(B.enc).to(dev)
    moved = B.units.copy()
    moved["in_off"] += np.uint64(shift)
    units_dev = device.units_to_device(moved, dev)
    table = device.UnitTable(dictionary, big, units_dev, len(moved), B.total)
    try:
        for through_table in (False, True):
            out_dev = torch.full((B.total,), -1, dtype=torch.int32, device=dev)
            end_dev = torch.zeros(len(moved), dtype=torch.int64, device=dev)
            if through_table:
                table.decode(out_dev, end_dev)
            else:
                dictionary.decode_units(big, units_dev, len(moved), out_dev, end_dev)
            torch.cuda.synchronize()
            got = out_dev.cpu().numpy().view(np.uint32)
            for u, (at, want) in enumerate(B.expect):
                assert np.array_equal(got[at:at + len(want)], want), (u, through_table)
                assert (got[at + len(want):at + len(want) + SB.CANARY] == 0xFFFFFFFF).all(), (u, through_table)
            assert np.array_equal(end_dev.cpu().numpy().view(np.uint64), B.ends + np.uint64(shift)), through_table
    finally:
        table.close()
        del big
        torch.cuda.empty_cache()
