"""Unit and block tables in the shapes callers make (tests/table_shapes.py) decode exactly on the device: permuted,
reversed, subsets with compacted outputs, scattered outputs with holes, every entry twice, whole lists beside pieces, and
— single-dictionary streams — a whole list followed by its own later pieces (a unit whose next table entry starts inside
its bytes). Integers, docIDs, freqs and end offsets bit for bit, canaries in front, behind and in every hole, through
dint_decode_units, prepared unit tables, the one-shot block call and prepared block tables (untaught and taught), under a
covering list of the library's switches."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import fuzz_streams as F
import table_shapes as TS

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_digests.json")))
VROOM = F.plan(*GOLDEN["vroom_plan"])
INDEX = F.index_plan(*GOLDEN["index_plan"])
QUERY = F.query_plan(*GOLDEN["query_plan"])
N_V, N_I, N_Q = GOLDEN["vroom_plan"][0], GOLDEN["index_plan"][0], GOLDEN["query_plan"][0]
# two cases per dictionary kind (plan order: single, rectangular, multi)
V_CASES = [VROOM[N_V * k + i] for k, pick in enumerate(((3, 8), (3, 8), (4, 8))) for i in pick]
B_CASES = [c for k in range(3) for c in (INDEX[N_I * k + 1], QUERY[N_Q * k + 1])]
# settings of the switches, dealt to the (case, shape) pairs in turn: every non-default value meets every kind it affects
U_SETTINGS = [{}, {"bundles": 0}, {"chunk_split": 0}, {"chunk_split": 2}, {"chunk_split": 4}]
B_SETTINGS = [{}, {"index_concurrent": 0}, {"index_pair": 0}, {"index_inline_tails": 0}, {"bundles": 0},
              {"chunk_split": 0}, {"chunk_split": 2}, {"chunk_split": 4}]
CANARIES = (0xFFFFFFFF, 0x5A5A5A5A)
GUARD = 64


def _unit_params():
    out = []
    for ci, case in enumerate(V_CASES):
        names = TS.UNIT_SHAPES + (TS.OVERLAP_SHAPES if case[1] != F.MULTI else ())
        for si, name in enumerate(names):
            out.append(pytest.param(case, name, U_SETTINGS[(ci + si) % len(U_SETTINGS)],
                                    id=f"seed{case[0]}-{name}"))
    return out


def _block_params():
    out = []
    for ci, case in enumerate(B_CASES):
        for si, name in enumerate(TS.BLOCK_SHAPES):
            out.append(pytest.param(case, name, B_SETTINGS[(ci + si) % len(B_SETTINGS)],
                                    id=f"seed{case[0]}-{name}"))
    return out


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev  # fails loudly if libdint_hip.so is missing

    return dev


@pytest.fixture(autouse=True)
def reset_options(device):
    yield
    device.reset_options()


def _one_case(build):
    """The tests of a case run one after the other: keep the last case built (its dictionaries and device buffers)."""
    last = {}

    def get(case):
        if last.get("seed") != case[0]:
            last.clear()
            last["value"], last["seed"] = build(case), case[0]
        return last["value"]

    return get


def build_unit_case(case):
    """-> (FuzzDictionary, FuzzStream, Dictionary, the stream on the device, {name: UnitShape})"""
    import torch
    from dint_amd import device

    D, S = F.build_case(case)
    d = device.Dictionary(D.kind, D.file)
    cuts = ()
    if D.kind != F.MULTI:  # the mixed shape's block-sized pieces and more overlap pairs: dint_index_stream's own cuts
        cuts = tuple(d.index_stream(S.enc, u)[0] for u in (256, 77))
    return D, S, d, torch.from_numpy(np.ascontiguousarray(S.enc)).to("cuda:0"), TS.unit_shapes(S, D.kind, case[0], cuts)


def build_block_case(case, build=F.build_index_case):
    """-> (docs Dictionary, freqs Dictionary, the padded index, it on the device, {name: BlockShape})"""
    import torch
    from dint_amd import device

    Dd, Df, X = build(case)
    blocks, total = device.index_posting_lists(X.index, X.offsets)
    assert total == len(X.docids) and np.array_equal(blocks, TS.block_table(X))
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    padded = np.concatenate([X.index, np.zeros(16, np.uint8)])
    return dd, fd, padded, torch.from_numpy(padded).to("cuda:0"), TS.block_shapes(X, blocks, case[0])


_unit_case = _one_case(build_unit_case)
_block_case = _one_case(lambda case: build_block_case(case, F.build_query_case if case in QUERY else F.build_index_case))


def _buffer(n, canary):
    import torch

    return torch.full((GUARD + n + GUARD,), np.int32(np.uint32(canary).view(np.int32)).item(), dtype=torch.int32,
                      device="cuda:0")


def _check_output(buf, want, hole, canary, what, starts=None, free=None):
    """The whole buffer: guards and holes hold the canary, entries their integers (except where `free`)."""
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:GUARD] == canary).all() and (got[-GUARD:] == canary).all(), f"{what}: wrote outside its buffer"
    full = np.where(hole, np.uint32(canary), want)
    differ = got[GUARD:-GUARD] != full
    if free is not None:
        differ &= ~free
    bad = np.flatnonzero(differ)
    if bad.size:
        at = int(bad[0])
        where = "a hole" if hole[at] else "an entry"
        if starts is not None and not hole[at]:
            where = f"entry {int(np.searchsorted(starts[0], at, side='right') - 1)} of the output-sorted table"
        raise AssertionError(f"{what}: {bad.size} integers differ, the first at {at} ({where}): "
                             f"{got[GUARD + at]:#x} != {full[at]:#x}")


def _decode_units_checked(shape, decode, what):
    """decode(out_view, end_view) twice, canaries of two values: integers, holes, guards and end offsets. A unit that a later
    entry begins inside of (TS.cut_into: outside the contract of dint_decode_units) may decode wrong, but only inside its
    own [out_off, out_off + n); every other unit stays exact."""
    import torch

    order = np.argsort(shape.units["out_off"], kind="stable")
    starts = (shape.units["out_off"][order].astype(np.int64),)
    cut = TS.cut_into(shape)
    free = np.zeros(shape.capacity, dtype=bool)
    for i in np.flatnonzero(cut):
        free[int(shape.units["out_off"][i]): int(shape.units["out_off"][i]) + int(shape.units["n"][i])] = True
    for canary in CANARIES:
        out = _buffer(shape.capacity, canary)
        ends = torch.full((len(shape.units),), -1, dtype=torch.int64, device="cuda:0")
        decode(out[GUARD:GUARD + shape.capacity], ends)
        torch.cuda.synchronize()
        _check_output(out, shape.want, shape.hole, canary, what, starts, free)
        got = ends.cpu().numpy().view(np.uint64)
        bad = np.flatnonzero((got != shape.ends) & ~cut)
        assert bad.size == 0, f"{what}: {bad.size} end offsets differ, unit {bad[0]}: {got[bad[0]]} != {shape.ends[bad[0]]}"


def check_unit_shape(device, kind, d, enc_dev, sh, what=""):
    """dint_decode_units and prepared tables (multi: split_units and refine_units each on and off) over one shape."""
    units_dev = device.units_to_device(sh.units, enc_dev.device)
    n = len(sh.units)
    _decode_units_checked(sh, lambda out, ends: d.decode_units(enc_dev, units_dev, n, out, ends), f"{sh.name}: decode_units {what}")
    for split, refine in [(1, 1), (0, 1), (1, 0), (0, 0)] if kind == F.MULTI else [(1, 1)]:
        with device.options(split_units=split, refine_units=refine):
            table = device.UnitTable(d, enc_dev, units_dev, n, sh.capacity)
            try:
                _decode_units_checked(sh, lambda out, ends: table.decode(out, ends),
                                      f"{sh.name}: UnitTable {what} split_units={split} refine_units={refine}")
            finally:
                table.close()


@pytest.mark.parametrize("case,name,setting", _unit_params())
def test_unit_table_shape(device, case, name, setting):
    D, S, d, enc_dev, shapes = _unit_case(case)
    assert (name == "overlapping") == TS.cut_into(shapes[name]).any()  # (the overlapping shape is not vacuous)
    with device.options(**setting):
        check_unit_shape(device, D.kind, d, enc_dev, shapes[name], str(setting))


def _one_shot(device, dd, fd, index_dev, index_bytes, blocks_dev, n_blocks, docids, freqs, capacity):
    import torch

    device._check(device._lib.dint_decode_posting_blocks(
        dd._h, fd._h if fd is not None else None, index_dev.data_ptr(), index_bytes, blocks_dev.data_ptr(), n_blocks,
        docids.data_ptr(), freqs.data_ptr() if freqs is not None else None, capacity,
        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "dint_decode_posting_blocks")
    torch.cuda.synchronize()


def check_block_shape(device, dd, fd, padded, index_dev, sh, what=""):
    """The one-shot call (with and without freqs), an untaught table (three decodes, then docs only: what it has learnt
    agrees with what it was given) and a taught one (learn) over one shape."""
    import torch

    cap, nb = sh.capacity, len(sh.blocks)
    blocks_dev = torch.from_numpy(np.ascontiguousarray(sh.blocks).view(np.uint8).copy()).to("cuda:0")

    def run(decode, with_freqs, canary, how):
        docids, freqs = _buffer(cap, canary), _buffer(cap, canary)
        decode(docids[GUARD:GUARD + cap], freqs[GUARD:GUARD + cap] if with_freqs else None)
        torch.cuda.synchronize()
        _check_output(docids, sh.docids, sh.hole, canary, f"{sh.name}: {how} {what} docIDs")
        if with_freqs:
            _check_output(freqs, sh.freqs, sh.hole, canary, f"{sh.name}: {how} {what} freqs")
        else:
            assert (freqs.cpu().numpy().view(np.uint32) == canary).all(), f"{sh.name}: {how} {what}: a docs-only decode wrote freqs"

    for canary, with_freqs in zip(CANARIES, (True, False)):
        run(lambda o, f: _one_shot(device, dd, fd if f is not None else None, index_dev, padded.size, blocks_dev, nb, o, f, cap),
            with_freqs, canary, "one-shot")
    plain, taught = device.BlockTable(dd, sh.blocks, padded.size), device.BlockTable(dd, sh.blocks, padded.size)
    try:
        taught.learn(dd, fd, index_dev, padded.size)
        # untaught: learns under its first two decodes, the third is the one-launch form; then a docs-only decode
        for p in range(4):
            run(lambda o, f: plain.decode(dd, fd if f is not None else None, index_dev, padded.size, o, f), p < 3,
                CANARIES[p % 2], f"untaught decode {p + 1}")
            if p == 2:
                info = plain.info()
                full = int((sh.blocks["n"] == 256).sum())
                assert info["n_blocks"] == nb and info["n_short_blocks"] == nb - full, info
                assert info["complete_decodes"] == 3 and info["spans_exact"] == 1 and info["freqs_units_ready"] == 1, info
                kept = int(device.get_option("bundles") != 0)  # (bundles=0: no bundle schedule to keep)
                assert info["docs_schedule"] == kept and info["freqs_schedule"] == kept, info
                assert info["docs_queue_items"] <= full and info["freqs_queue_items"] <= full, info
                assert (info["short_block_tickets"] > 0) == (nb > full), info
                assert not plain.ready(True) or plain.ready(False)
        for p in range(2):
            run(lambda o, f: taught.decode(dd, fd if f is not None else None, index_dev, padded.size, o, f), p == 0,
                CANARIES[p], f"taught decode {p + 1}")
        # the schedules learnt at set-up are the ones three decodes learn
        ti, pi = taught.info(), plain.info()
        for k in ("n_blocks", "n_short_blocks", "spans_exact", "docs_schedule", "freqs_schedule", "docs_queue_items",
                  "freqs_queue_items", "short_block_tickets"):
            assert ti[k] == pi[k], (sh.name, k, ti, pi)
        assert taught.ready(True) == plain.ready(True) and taught.ready(False) == plain.ready(False)
    finally:
        plain.close()
        taught.close()


@pytest.mark.parametrize("case,name,setting", _block_params())
def test_block_table_shape(device, case, name, setting):
    dd, fd, padded, index_dev, shapes = _block_case(case)
    with device.options(**setting):
        check_block_shape(device, dd, fd, padded, index_dev, shapes[name], str(setting))
