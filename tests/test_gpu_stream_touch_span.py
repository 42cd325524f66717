"""The stream touch sized by each unit's bytes (kernels/bundles.inc decode_unit_single, kernels/segment.inc TOUCH; the rule:
dint_stream_touch.hpp stream_touch_span / unit_stream_span, pinned case by case in tests/test_stream_touch_span_cpu.py): a unit's
window is the lines from tile 3's first byte through its own last byte — the next record of the table says where that is — up
to 128 of them, the lines from the 64th on by a second load in the same trip. The loads' values are used for nothing, so what
can go wrong is an address or a record read past the table: these are the smallest shapes at which the window has 64 lines
against 65, at which the cap of 128 binds, at which either load meets the end of the buffer or offset 2^32, and the tables
whose next record says nothing (reverse order, a record twice: the rule of n) or too much (every other unit left out: cut to
6 n bytes and the cap). Streams are assembled slot by slot with tests/test_gpu_stream_bursts.py's pieces, every one decoded
through dint_decode_units and through a prepared UnitTable, integers and end offsets bit for bit against the assembler's input,
canary words behind every unit's output, the device copy of a stream exactly as long as the stream. No test looks for a fault:
the bounds are the CPU cases'."""
import numpy as np
import pytest

import fuzz_streams as F
import test_gpu_stream_bursts as SB

pytestmark = pytest.mark.gpu

LINE = 128
PROLOGUE = 1536
ONE_LOAD = PROLOGUE + 64 * LINE  # 9728: a unit that begins a line and spans this much has a window of exactly 64 lines


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev  # fails loudly if libdint_hip.so is missing

    return dev


@pytest.fixture(scope="module")
def fuzz_dict():
    D = F.make_dictionary(np.random.default_rng(77002), F.SINGLE, m_entries=65536, value_profile="mixed", size_profile="pow2")
    assert {1, 2, 4, 16} <= set(D.by_size[0])
    return D


@pytest.fixture(scope="module")
def dictionary(device, fuzz_dict):
    return device.Dictionary(fuzz_dict.kind, fuzz_dict.file)


def exact(r, D, n, n_bytes):
    """A unit of EXACTLY n integers in EXACTLY n_bytes stream bytes: one-slot codewords of 4, 2 and 1 integers (and as many of 16
    as a dense unit needs), shuffled."""
    all_slots = n_bytes // 2
    assert n_bytes % 2 == 0 and all_slots <= n <= 16 * all_slots
    w = max(0, -(-(n - 4 * all_slots) // 12))  # codewords of 16: the rest decodes to at most 4 integers a slot
    slots, m = all_slots - w, n - 16 * w
    x = (m - slots) // 3          # 4 x + 2 y + z = m, x + y + z = slots
    y = (m - slots) - 3 * x
    z = slots - x - y
    assert min(x, y, z) >= 0
    ids = np.concatenate([r.choice(D.by_size[0][s], c) for s, c in ((16, w), (4, x), (2, y), (1, z))]).astype(np.int64)
    r.shuffle(ids)
    assert int(D.size[0][ids].sum()) == n and len(ids) == all_slots
    return ids, np.zeros(all_slots, dtype=np.int64)


def sparse(r, D, n, exc_p=0.25):
    """A unit of n integers from codewords of one and two integers and exceptions: about two stream bytes an integer."""
    ids, lits, have = [], [], 0
    pool = np.concatenate([D.by_size[0][1], D.by_size[0][2]])
    while have < n:
        if n - have < 4:
            i, lit = int(r.choice(D.by_size[0][1])), 0
        elif r.random() < exc_p:
            i = int(r.integers(0, 2))
            lit = int(r.integers(0, 1 << (16 if i == 0 else 32)))
        else:
            i, lit = int(r.choice(pool)), 0
        ids.append(i)
        lits.append(lit)
        have += int(D.size[0][i])
    assert have == n
    return np.array(ids, dtype=np.int64), np.array(lits, dtype=np.int64)


def tiny(r, D, n):
    return r.choice(D.by_size[0][1], n).astype(np.int64), np.zeros(n, dtype=np.int64)


def span_of(B, u):
    return int(B.ends[u]) - int(B.units["in_off"][u])


def placements(r, D, unit, res):
    """The unit as the stream's last (the buffer ends with it), behind another long unit, and with a unit of one integer behind it
    whose two bytes end the stream."""
    last = SB.assemble(D, [unit], residues=[res])
    assert int(last.ends[-1]) == last.enc.size
    behind = SB.assemble(D, [exact(r, D, 16384, 7000), unit], residues=[5, res])
    assert int(behind.ends[-1]) == behind.enc.size
    followed = SB.assemble(D, [unit, tiny(r, D, 1)], residues=[res, (res + span_of(last, 0)) % 128])
    assert list(followed.units["n"])[1] == 1 and int(followed.units["in_off"][1]) == followed.enc.size - 2 == int(followed.ends[0])
    return last, behind, followed


@pytest.mark.parametrize("res", [0, 1, 127])
@pytest.mark.parametrize("delta", [-2, 0, 2], ids=["under", "at", "over"])
def test_one_load_against_two(device, dictionary, fuzz_dict, res, delta):
    """16384 integers whose stream ends just under, at and just over 1536 + 8192 bytes past their line offset: 64 lines — one
    load — up to the byte count that fills them, 65 — the second load, all its lanes on one line — from the next slot on."""
    r = np.random.default_rng(1000 + 3 * res + delta)
    line_off = (res + PROLOGUE) % LINE  # tile 3's first byte inside its line
    fills = ONE_LOAD - line_off     # the byte count that fills the 64 lines (a stream of 16-bit slots has the even ones)
    unit = exact(r, fuzz_dict, 16384, fills - fills % 2 + delta)
    for B in placements(r, fuzz_dict, unit, res):
        u = int(np.flatnonzero(B.units["n"] == 16384)[-1])
        first_line = (int(B.units["in_off"][u]) + PROLOGUE) // LINE
        assert (int(B.ends[u]) - 1) // LINE - first_line + 1 == (65 if delta > 0 else 64)
        SB.check(device, dictionary, B)


@pytest.mark.parametrize("res", [0, 77])
def test_a_unit_of_32_kb_where_the_cap_binds(device, dictionary, fuzz_dict, res):
    r = np.random.default_rng(2000 + res)
    unit = sparse(r, fuzz_dict, 16384)
    for B in placements(r, fuzz_dict, unit, res):
        u = int(np.flatnonzero(B.units["n"] == 16384)[-1])
        assert span_of(B, u) > PROLOGUE + 128 * LINE + 8192 and span_of(B, u) <= 6 * 16384  # about 32 KB: half of it behind the window
        SB.check(device, dictionary, B)


def long_units(r, D, spans):
    return [exact(r, D, 16384, s) if s else sparse(r, D, 16384) for s in spans]


SPANS = [6000, 9726, 9728, 9730, 13800, 17100, 0, 7600]  # 0: a sparse unit of about 32 KB


def test_tables_whose_next_record_says_nothing(device, dictionary, fuzz_dict):
    """A table in reverse order — every next record begins below its unit — and a table with records repeated — the next record
    begins where its unit does: the span is not known and the window is the rule of n's. (The repeated records decode the same
    integers to the same place twice.)"""
    r = np.random.default_rng(31)
    parts = long_units(r, fuzz_dict, SPANS) + [exact(r, fuzz_dict, 3000, 2000), tiny(r, fuzz_dict, 1)]
    B = SB.assemble(fuzz_dict, parts, residues=[(53 * j) % 128 for j in range(len(parts))])
    units, ends = B.units.copy(), B.ends.copy()
    B.units, B.ends = units[::-1].copy(), ends[::-1].copy()
    assert np.all(np.diff(B.units["in_off"].astype(np.int64)) < 0)
    SB.check(device, dictionary, B)
    twice = np.array([0, 1, 1, 2, 3, 3, 3, 4, 5, 6, 6, 7, 8, 9, 9])
    B.units, B.ends = units[twice].copy(), ends[twice].copy()
    SB.check(device, dictionary, B)


def test_a_partial_table_that_skips_every_other_unit(device, dictionary, fuzz_dict):
    """The next record is two units on: spans twice as long as the units, cut by 6 n bytes and by the cap — lines of the units that
    the table leaves out, all of them inside the stream. The outputs of the units left out stay as they were."""
    r = np.random.default_rng(41)
    parts = long_units(r, fuzz_dict, SPANS + SPANS[::-1]) + [exact(r, fuzz_dict, 2600, 1538), exact(r, fuzz_dict, 2600, 1538), tiny(r, fuzz_dict, 3)]
    for keep in (slice(0, None, 2), slice(1, None, 2)):
        B = SB.assemble(fuzz_dict, parts, residues=[(29 * j + 1) % 128 for j in range(len(parts))])
        B.units, B.ends, B.expect = B.units[keep].copy(), B.ends[keep].copy(), B.expect[keep]
        SB.check(device, dictionary, B)
    # ... and a scattered one: the records that are kept, in another order (some next records ahead, some behind)
    B = SB.assemble(fuzz_dict, parts, residues=[(29 * j + 1) % 128 for j in range(len(parts))])
    order = np.random.default_rng(42).permutation(len(parts))[:11]
    B.units, B.ends, B.expect = B.units[order].copy(), B.ends[order].copy(), [B.expect[j] for j in order]
    SB.check(device, dictionary, B)


def test_a_scheduled_launch_with_tiny_units_between_the_long_ones(device, dictionary, fuzz_dict):
    """More long units than a workgroup has waves, two to five tiny units between them: the launch is scheduled, the tiny units are
    bundled, and "the next record" of a queue item is a bundled unit — the long unit's span ends where the first tiny one begins."""
    r = np.random.default_rng(51)
    parts = []
    for j in range(40):
        parts.append(exact(r, fuzz_dict, 16384, [5800, 9728, 9730, 12000, 17000][j % 5]) if j % 8 else sparse(r, fuzz_dict, 16384))
        parts += [tiny(r, fuzz_dict, int(r.integers(1, 60))) for _ in range(2 + j % 4)]
    B = SB.assemble(fuzz_dict, parts)  # (no filler: every unit begins where the one before ends)
    assert int((B.units["n"] == 16384).sum()) == 40 and int((B.units["n"] < 64).sum()) > 100
    SB.check(device, dictionary, B)
    B = SB.assemble(fuzz_dict, parts, residues=[(37 * j) % 128 for j in range(len(parts))], tail_pad=3)
    SB.check(device, dictionary, B)


@pytest.mark.parametrize("cut", [PROLOGUE + 64 * LINE + 2000, 17000 + 19 + PROLOGUE + 100 * LINE])
def test_a_stream_placed_across_4_gib(device, dictionary, fuzz_dict, cut):
    """The stream's byte `cut` at offset 2^32 of a 4.3 GB buffer that ends with the stream: 2^32 falls inside the lines of the
    second load of the first unit (15 lines in), and of the second unit, whose window the cap ends. The window's first line, the
    room left and the span are 64-bit until they are cut."""
    import torch

    r = np.random.default_rng(cut)
    parts = [exact(r, fuzz_dict, 16384, 17000), sparse(r, fuzz_dict, 16384), exact(r, fuzz_dict, 16384, 13800), tiny(r, fuzz_dict, 2)]
    B = SB.assemble(fuzz_dict, parts, residues=[0, 19, 64, 127])
    u = 0 if cut < 17000 else 1
    line0 = (int(B.units["in_off"][u]) + PROLOGUE) // LINE * LINE
    assert line0 + 64 * LINE < cut < min(line0 + 128 * LINE, int(B.ends[u]))
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
            for k, (at, want) in enumerate(B.expect):
                assert np.array_equal(got[at:at + len(want)], want), (k, through_table)
                assert (got[at + len(want):at + len(want) + SB.CANARY] == 0xFFFFFFFF).all(), (k, through_table)
            assert np.array_equal(end_dev.cpu().numpy().view(np.uint64), B.ends + np.uint64(shift)), through_table
    finally:
        table.close()
        del big
        torch.cuda.empty_cache()
