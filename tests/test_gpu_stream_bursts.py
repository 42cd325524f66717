"""The single-dictionary segment loop asks for its slots two tiles at a time (kernels/segment.inc, DINT_SLOT_BURST): the
smallest shapes at which that loop can go wrong. A tile is 256 16-bit slots (512 stream bytes); the prologue asks for tiles
0, 1 and 2, every odd tile t for the pair t+2, t+3. Streams are assembled slot by slot with tests/fuzz_streams.py's pieces, the
expected integers are its substitution; every stream is decoded through dint_decode_units and through a prepared UnitTable
into a buffer with canary words behind every unit, and the device copy of a stream is exactly as long as the stream.

* units of 1 to 6 tiles: 256 k - 1, 256 k and 256 k + 1 slots — both parities, a unit that ends on the first and on the second
  tile of a pair, a unit of one tile;
* unit starts at every residue of in_off mod 128 (so every byte alignment of the loads);
* a last unit whose payload ends on the stream's final byte, the stream's length no multiple of 8: the end-of-buffer path
  of either load of a pair;
* a stream shorter than a tile, shorter than 128 bytes, of 8 bytes;
* exception markers in the last slots of a tile, their literals in (or straddling into) the next tile, at every tile
  boundary of a 7-tile unit: inside a pair, between two pairs and between the prologue's tiles and the first pair;
* a small posting-list index through dint_decode_block_table: the in-index kernels run the same loop over one-tile blocks."""
import numpy as np
import pytest

import fuzz_streams as F

pytestmark = pytest.mark.gpu

TILE = 256  # slots
CANARY = 4  # words behind every unit's output


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev  # fails loudly if libdint_hip.so is missing

    return dev


@pytest.fixture(scope="module")
def fuzz_dict():
    # 65536 entries of 1 to 16 integers: hot and cold codewords, heads and tails, wide values
    return F.make_dictionary(np.random.default_rng(424242), F.SINGLE, m_entries=65536, value_profile="mixed", size_profile="pow2")


@pytest.fixture(scope="module")
def dictionary(device, fuzz_dict):
    return device.Dictionary(fuzz_dict.kind, fuzz_dict.file)


def craft(r, D, n_slots, exceptions=None, exc_p=0.03):
    """Codewords that take EXACTLY n_slots 16-bit slots: `exceptions` {slot position: (marker, literal)} where given, random
    exceptions (with probability exc_p a codeword) elsewhere, one-slot codewords of any id (runs included) otherwise."""
    exceptions = exceptions or {}
    ids, lits = [], []
    pos = 0
    while pos < n_slots:
        if pos in exceptions:
            marker, lit = exceptions[pos]
        elif r.random() < exc_p:
            marker = int(r.integers(0, 2))
            lit = int(r.integers(0, 1 << (16 if marker == 0 else 32)))
        else:
            marker, lit = None, 0
        width = 1 if marker is None else 2 + marker
        # a random exception must neither run over the end nor over a placed one
        if marker is not None and pos not in exceptions and (pos + width > n_slots or any(pos < p < pos + width for p in exceptions)):
            marker, lit, width = None, 0, 1
        assert pos + width <= n_slots
        ids.append(int(r.integers(2, len(D.size[0]))) if marker is None else marker)
        lits.append(lit)
        pos += width
    return np.array(ids, dtype=np.int64), np.array(lits, dtype=np.int64)


class Built:
    def __init__(self, enc, units, ends, expect, total):
        self.enc, self.units, self.ends, self.expect, self.total = enc, units, ends, expect, total


def assemble(D, parts, residues=None, tail_pad=0):
    """A stream of one unit per (ids, lits) in `parts`, unit u starting at a byte offset = residues[u] mod 128 (filler
    bytes of 0xA5 between the units — what a list header or another list's bytes would be); outputs CANARY words apart."""
    chunks, units, ends, expect = [], [], [], []
    pos = out = 0
    for u, (ids, lits) in enumerate(parts):
        if residues is not None:
            pad = (residues[u] - pos) % 128
            chunks.append(np.full(pad, 0xA5, dtype=np.uint8))
            pos += pad
        body, _ = F.slot_bytes(ids, lits)
        want = F.expand(D, 0, ids, lits)
        units.append((pos, out, len(want), u))
        chunks.append(body)
        pos += len(body)
        ends.append(pos)
        expect.append((out, want))
        out += len(want) + CANARY
    chunks.append(np.full(tail_pad, 0xA5, dtype=np.uint8))
    return Built(np.concatenate(chunks), np.array(units, dtype=F.UNIT_DTYPE), np.array(ends, dtype=np.uint64), expect, out)


def check(device, d, B):
    import torch

    dev = torch.device("cuda", 0)
    enc_dev = torch.from_numpy(np.ascontiguousarray(B.enc)).to(dev)
    assert enc_dev.numel() == B.enc.size  # the device buffer ends where the stream ends
    units_dev = device.units_to_device(B.units, dev)
    table = device.UnitTable(d, enc_dev, units_dev, len(B.units), B.total)
    try:
        for through_table in (False, True):
            out_dev = torch.full((B.total,), -1, dtype=torch.int32, device=dev)
            end_dev = torch.zeros(len(B.units), dtype=torch.int64, device=dev)
            if through_table:
                table.decode(out_dev, end_dev)
            else:
                d.decode_units(enc_dev, units_dev, len(B.units), out_dev, end_dev)
            torch.cuda.synchronize()
            got = out_dev.cpu().numpy().view(np.uint32)
            for u, (at, want) in enumerate(B.expect):
                bad = np.flatnonzero(got[at:at + len(want)] != want)
                assert bad.size == 0, f"unit {u} (table {through_table}): integer {bad[0]}: {got[at + bad[0]]} != {want[bad[0]]}"
                assert (got[at + len(want):at + len(want) + CANARY] == 0xFFFFFFFF).all(), f"unit {u}: wrote behind its output"
            assert np.array_equal(end_dev.cpu().numpy().view(np.uint64), B.ends), through_table
    finally:
        table.close()


SLOT_COUNTS = [TILE * k + e for k in range(1, 7) for e in (-1, 0, 1)]


def test_units_of_one_to_six_tiles_at_every_start_residue(device, dictionary, fuzz_dict):
    r = np.random.default_rng(1)
    parts, residues = [], []
    for res in range(128):  # every residue once, the slot counts going round (128 = 7 * 18 + 2)
        parts.append(craft(r, fuzz_dict, SLOT_COUNTS[res % len(SLOT_COUNTS)]))
        residues.append(res)
    for i, s in enumerate(SLOT_COUNTS):  # every slot count at an odd and at an even residue that it did not have above
        parts.append(craft(r, fuzz_dict, s))
        residues.append((37 * i + 64) % 128)
    check(device, dictionary, assemble(fuzz_dict, parts, residues, tail_pad=3))


@pytest.mark.parametrize("lead", [1, 3, 6])
def test_the_last_unit_ends_on_the_streams_final_byte(device, dictionary, fuzz_dict, lead):
    """One stream per slot count: a one-tile unit, then the unit under test, nothing behind it. `lead` filler bytes in front
    make the stream's length odd / no multiple of 8, 128 or 512 for every slot count."""
    r = np.random.default_rng(2 + lead)
    for s in SLOT_COUNTS:
        # (no exception behind the last codeword: the final slot is a codeword's)
        parts = [craft(r, fuzz_dict, 200), craft(r, fuzz_dict, s)]
        B = assemble(fuzz_dict, parts, residues=[lead, (lead + 400 + 2 * s) % 128 | 1])
        assert int(B.ends[-1]) == B.enc.size and B.enc.size % 8 != 0 and B.enc.size % 2 == 1, (s, B.enc.size)
        check(device, dictionary, B)


@pytest.mark.parametrize("n_slots", [4, 5, 40, 63, 64, 100, 255])
def test_a_stream_shorter_than_a_tile(device, dictionary, fuzz_dict, n_slots):
    """8, 10, 80, 126 and 128 bytes (shorter than a line), 200 and 510 (shorter than a tile): all three of the prologue's loads and
    whatever the loop asks for take the end-of-buffer path."""
    r = np.random.default_rng(100 + n_slots)
    B = assemble(fuzz_dict, [craft(r, fuzz_dict, n_slots)])
    assert B.enc.size == 2 * n_slots
    check(device, dictionary, B)


@pytest.mark.parametrize("flavour", ["e16_last_slot", "e32_last_slot", "e32_straddling"])
def test_exceptions_at_every_tile_boundary(device, dictionary, fuzz_dict, flavour):
    """A 7-tile unit (boundaries 1..6: tiles 0|1 and 1|2 are the prologue's, 2|3 prologue | first pair, 3|4 and 5|6 inside a
    pair, 4|5 between two pairs) with the marker in the last slot of the tile and its literal in the next one, or a 32-bit
    literal with a half on either side (the lane-0 read of the next tile's packed slots); literals below and above 65536."""
    r = np.random.default_rng({"e16_last_slot": 5, "e32_last_slot": 6, "e32_straddling": 7}[flavour])
    parts = []
    for rep in range(3):
        exc = {}
        for j in range(1, 7):
            if flavour == "e16_last_slot":
                exc[TILE * j - 1] = (0, int(r.integers(0, 1 << 16)))
            else:
                lit = int(r.integers(1 << 16, 1 << 32)) if (j + rep) % 2 else int(r.integers(0, 1 << 16))
                exc[TILE * j - (1 if flavour == "e32_last_slot" else 2)] = (1, lit)
        parts.append(craft(r, fuzz_dict, 7 * TILE - rep, exc, exc_p=0.0 if rep == 0 else 0.03))
    # odd unit starts, so that the literals sit at odd addresses too
    check(device, dictionary, assemble(fuzz_dict, parts, residues=[0, 77, 127], tail_pad=5))


def test_an_in_index_posting_list_index(device):
    """Blocks of 256 postings (one tile, or two when a block is full of exceptions) through dint_decode_block_table, docs and
    freqs: the in-index kernels share the single-dictionary segment loop."""
    import torch

    r = np.random.default_rng(9)
    Dd = F.make_dictionary(r, F.SINGLE, m_entries=5000, value_profile="byte_edge", size_profile="pow2", nest_p=0.4)
    Df = F.make_dictionary(r, F.SINGLE, m_entries=65536, value_profile="mixed", size_profile="any")
    X = F.make_index(r, Dd, Df, 60)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    blocks, total = device.index_posting_lists(X.index, X.offsets)
    assert total == len(X.docids)
    dev = torch.device("cuda", 0)
    padded = np.concatenate([X.index, np.zeros(16, np.uint8)])
    index_dev = torch.from_numpy(padded).to(dev)
    table = device.BlockTable(dd, blocks, padded.size)
    try:
        for _ in range(2):
            docids_dev = torch.full((total + 64,), -1, dtype=torch.int32, device=dev)
            freqs_dev = torch.full((total + 64,), -1, dtype=torch.int32, device=dev)
            table.decode(dd, fd, index_dev, padded.size, docids_dev[:total], freqs_dev[:total])
            torch.cuda.synchronize()
            got = docids_dev.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:total], X.docids) and (got[total:] == 0xFFFFFFFF).all()
            got = freqs_dev.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:total], X.freqs) and (got[total:] == 0xFFFFFFFF).all()
    finally:
        table.close()
