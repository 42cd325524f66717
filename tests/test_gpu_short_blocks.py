"""The short (binary-interpolative) blocks on the GPU at their edges: the cases of tests/short_blocks.py — every length 1 .. 255,
code widths up to 825 bytes a docs part, every (value, range) pair around read_int's extra bit, tails behind full blocks up to
docID 0xFFFFFFFE, block tables around every ticket cut — through every way the device decodes them, against the encoder's input
(which tests/test_short_blocks_cpu.py shows the C oracle and tests/pydecode.py to decode the indexes to). Everything is compared
exactly: docIDs, freqs and consumed bytes as integers, ranked scores as bit patterns against the binary32 models
(tests/ranked.py, tests/ranked_or.py). Output buffers are poisoned and have canaries in front and behind.

Which decoder a call reaches (kernels/index.inc; hip_api_index.inc, hip_api_query.inc, hip_api_query_and.inc):
 * the lane decoder (interpolative_prefix_sums, one block a lane) in interpolative_tails_kernel: the one-shot call, block tables
   with index_inline_tails=0, dint_decode_block_host, dint_list_cache_create — and, in every query call under every option set,
   the FREQS parts (and_freqs_pass, the ranked calls) and both parts of an OR call's pages (decode_pages);
 * the same routine in tails_phase (tickets): the docs launch of a created block table, index_inline_tails=1;
 * an AND call's DOCS parts (candidate pages and probed pages, decode_pages_counted), by option set of FORMS:
     {}                                                     interpolative_block_wave (a single query: the one-launch form; a batch
                                                            of counts: the workgroup-per-query form; with freqs: the lean decode)
     query_batch_fused=0                                    interpolative_block_wave (a round per launch)
     query_fused_pages=0, query_tail_pages=0                interpolative_block_wave (the lean decode alone)
     query_lean_pages=0                                     the lane decoder in fix_pages_kernel (three launches)
     query_fused_copy=0, query_fused_pages=8, query_tail_pages=16   interpolative_block_wave (the one-launch form, inputs copied)
     query_or_pass_pages=1                                  interpolative_block_wave; the OR calls a page at a time
     query_or_pass_pages=5, query_lean_pages=1              the lane decoder in fix_pages_kernel (no decode is below one page)

The `wide` index is handed over at its exact size, with bytes that are not zero behind it in the buffer: its last list is 255
postings over the whole docID range, so both bit readers meet the end of the index in the middle of a word."""
import ctypes as C
import functools

import numpy as np
import pytest

import ranked
import ranked_or
import short_blocks as SB
import table_shapes as TS
from dint_amd import host
from or_union import union_freqs
from queries import intersect_freqs
from test_gpu_query_high_docids import FORMS
from test_gpu_table_shapes import CANARIES, GUARD, _buffer, _check_output, _one_shot

pytestmark = pytest.mark.gpu

TABLE_SETTINGS = [{}, {"index_inline_tails": 0}, {"index_pair": 0}, {"index_concurrent": 0}]
K = 1024


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev  # fails loudly if libdint_hip.so is missing

    return dev


@pytest.fixture(autouse=True)
def _options_back_to_default(device):
    yield
    device.reset_options()


class OnDevice:
    """An index of tests/short_blocks.py with its dictionaries and its bytes on the device. The buffer is 16 bytes longer than
    the index; `wide` is decoded with index_bytes = its exact size (what lies behind is not zero), the others with the 16 bytes
    counted in, as everywhere else in the suite."""

    def __init__(self, device, which, kind):
        import torch

        self.ix = ix = SB.index(which, kind)
        self.dd, self.fd = device.Dictionary(kind, ix.docs_dict), device.Dictionary(kind, ix.freqs_dict)
        padded = np.concatenate([ix.index, np.full(16, 0xA5, np.uint8)])
        self.index_dev = torch.from_numpy(padded).to("cuda:0")
        self.index_bytes = ix.index.size if which == "wide" else padded.size
        self.total = int(ix.docids.size)


@functools.lru_cache(maxsize=None)
def _on_device(which, kind):
    from dint_amd import device

    return OnDevice(device, which, kind)


def _whole(ix):
    """The index's own block table as a shape: lists in order, outputs back to back"""
    return TS._block_shape("whole index", ix, ix.blocks, np.arange(len(ix.blocks)), ix.blocks["out_off"], int(ix.docids.size))


# ---- 1. the one-shot decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", SB.KINDS)
@pytest.mark.parametrize("which", SB.INDEXES)
def test_one_shot_decode(device, which, kind):
    c = _on_device(which, kind)
    ix = c.ix
    blocks, total = device.index_posting_lists(ix.index, ix.offsets)
    assert total == c.total and np.array_equal(blocks, ix.blocks)
    docids, freqs = device.decode_posting_lists(c.dd, c.fd, ix.index, blocks, total)
    assert np.array_equal(docids, ix.docids) and np.array_equal(freqs, ix.freqs)
    docids, freqs = device.decode_posting_lists(c.dd, None, ix.index, blocks, total)
    assert freqs is None and np.array_equal(docids, ix.docids)


# ---- 2. created block tables ------------------------------------------------------------------------------------------------
def _check_table(device, c, sh, what):
    """The one-shot call (docs + freqs, docs only), an untaught table (three decodes, then docs only) and a taught one (docs +
    freqs, docs only) over one table; what the tables say of their short blocks."""
    import torch

    cap, nb = sh.capacity, len(sh.blocks)
    blocks_dev = torch.from_numpy(np.ascontiguousarray(sh.blocks).view(np.uint8).copy()).to("cuda:0")
    dd, fd, index_dev, index_bytes = c.dd, c.fd, c.index_dev, c.index_bytes

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
        run(lambda o, f: _one_shot(device, dd, fd if f is not None else None, index_dev, index_bytes, blocks_dev, nb, o, f, cap),
            with_freqs, canary, "one-shot")
    short = int((sh.blocks["n"] < 256).sum())
    n_tickets = len(SB.tickets(sh.blocks)[1])
    assert (n_tickets != 0) == (short != 0)
    plain, taught = device.BlockTable(dd, sh.blocks, index_bytes), device.BlockTable(dd, sh.blocks, index_bytes)
    try:
        taught.learn(dd, fd, index_dev, index_bytes)
        for p in range(4):
            run(lambda o, f: plain.decode(dd, fd if f is not None else None, index_dev, index_bytes, o, f), p < 3,
                CANARIES[p % 2], f"untaught decode {p + 1}")
        for p in range(2):
            run(lambda o, f: taught.decode(dd, fd if f is not None else None, index_dev, index_bytes, o, f), p == 0,
                CANARIES[p], f"taught decode {p + 1}")
        for table in (plain, taught):
            info = table.info()
            assert info["n_blocks"] == nb and info["n_short_blocks"] == short, (sh.name, what, info)
            # A created table keeps its tickets whatever index_inline_tails says at the time (the option is read by each
            # decode; tests/test_gpu_table_shapes.py pins that too): as many as the model cuts, none without a short block.
            assert info["short_block_tickets"] == n_tickets, (sh.name, what, info)
    finally:
        plain.close()
        taught.close()


@pytest.mark.parametrize("setting", TABLE_SETTINGS, ids=lambda s: "-".join(f"{k}={v}" for k, v in s.items()) or "default")
@pytest.mark.parametrize("kind", SB.KINDS)
def test_created_block_tables(device, kind, setting):
    with device.options(**setting):
        for which in SB.INDEXES:
            c = _on_device(which, kind)
            _check_table(device, c, _whole(c.ix), f"{which} {setting}")
        for name, (ix, sh) in SB.cuts(kind).items():
            c = _on_device("len" if ix is SB.index("len", kind) else "wide", kind)
            assert c.ix is ix
            _check_table(device, c, sh, str(setting))


# ---- 3. the host calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_decode_block_host_over_every_block(device, kind):
    """dint_decode_block_host over every block of LEN and EDGE: the docs part with its sum, the freqs part with 0xFFFFFFFF,
    the consumed bytes the model's (0 for a docs part without bits), the two parts chained to the next list's offset. The
    buffer ends with the index: the last block's bytes are the call's last."""
    for which in ("len", "edge"):
        c = _on_device(which, kind)
        ix, parts = c.ix, SB.parts(which)
        assert len(parts) == len(ix.blocks)
        for b in range(len(ix.blocks)):
            r = ix.blocks[b]
            n, at = int(r["n"]), int(r["in_off"])
            docs, freqs = parts[b]
            got, used = device.decode_block(c.dd, ix.index, at, docs.sum, n)
            assert np.array_equal(got, docs.values) and used == docs.size, (which, ix.names[int(r["list"])], used, docs.size)
            got, used_f = device.decode_block(c.fd, ix.index, at + used, SB.FREQS_PART, n)
            assert np.array_equal(got, freqs.values) and used_f == freqs.size, (which, ix.names[int(r["list"])], used_f, freqs.size)
            assert at + used + used_f == int(ix.offsets[int(r["list"]) + 1])


CACHED = [("wide", f"tail {n}") for n in SB.TAIL_LENGTHS] + [("len", "len 1"), ("len", "len 5"), ("wide", "wide 255")]


@pytest.mark.parametrize("with_freqs_dict", [True, False])
@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_list_cache_over_short_and_tailed_lists(device, kind, with_freqs_dict):
    """dint_list_cache_*: every block's two parts, the consumed bytes chained through the list. `len 1` (one posting) and
    `len 5` (consecutive docIDs) have a docs part of 0 bytes: the freqs part starts where the docs part does, and only the part
    call (dint_list_cache_decode_part, which takes the Coder's sum_of_values) can tell them apart; the plain call answers with
    the docs part there. A cache made without a freqs dictionary refuses the freqs parts; an offset where no part starts is
    refused."""
    for which, name in CACHED:
        c = _on_device(which, kind)
        ix = c.ix
        i = ix.at[name]
        lo, hi = int(ix.offsets[i]), int(ix.offsets[i + 1])
        cache = device.ListCache(c.dd, c.fd if with_freqs_dict else None, ix.index[lo:hi])
        rows = ix.blocks_of(name)
        at = int(ix.blocks["in_off"][rows[0]]) - lo
        for b in rows:
            r = ix.blocks[b]
            n, out = int(r["n"]), int(r["out_off"])
            assert at == int(r["in_off"]) - lo
            want = ix.docids[out:out + n].astype(np.int64)
            gaps = (np.diff(np.r_[int(r["base"]) - 1, want]) - 1).astype(np.uint32)
            docs_sum = int(gaps.astype(np.int64).sum())
            got, used = cache.decode(at, n, docs_sum)
            assert np.array_equal(got, gaps), (name, int(b))
            got2, used2 = cache.decode(at, n)
            assert np.array_equal(got2, gaps) and used2 == used
            if n < 256:
                assert used == SB.parts(which)[int(b)][0].size
            end = SB.block_end(ix, int(b)) - lo
            if with_freqs_dict:
                got, used_f = cache.decode(at + used, n, SB.FREQS_PART)
                assert np.array_equal(got + np.uint32(1), ix.freqs[out:out + n]), (name, int(b))
                assert at + used + used_f == end, (name, int(b))
                if used != 0:  # (the plain call: where the offset says which part is meant)
                    got2, used2 = cache.decode(at + used, n)
                    assert np.array_equal(got2, got) and used2 == used_f
                    with pytest.raises(device.DintError):
                        cache.decode(at + used, n, docs_sum)          # no docs part starts there
                    with pytest.raises(device.DintError):
                        cache.decode(at, n, SB.FREQS_PART)            # no freqs part starts there
            else:
                with pytest.raises(device.DintError):
                    cache.decode(at + used, n, SB.FREQS_PART)
                if used != 0:
                    with pytest.raises(device.DintError):
                        cache.decode(at + used, n)
            if used > 1:
                with pytest.raises(device.DintError):
                    cache.decode(at + 1, n)
            with pytest.raises(device.DintError):
                cache.decode(at, n + 1 if n < 256 else 255)
            at = end
        assert at == hi - lo
        with pytest.raises(device.DintError):
            cache.decode(0, int(ix.blocks["n"][rows[0]]))  # the list's header: no part starts there
        cache.close()


def test_coder_walk_inside_a_list_scope_over_docs_parts_without_bytes(device, tmp_path):
    """The C++ surface of the same calls (dint/coders.hpp): tests/cpp/block_walker.cpp walks a list as the reference's
    document_enumerator does, inside a Coder::list_scope — Coder::decode for the docs part, then for the freqs part at the
    pointer the first call returned. For `len 1` and `len 5` that is the SAME pointer: the scope tells the parts apart by the
    call's sum_of_values."""
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "block_walker")
    subprocess.run(["g++", "-O1", "-std=c++17", f"-I{root}/include", f"-I{root}/dint_amd/csrc/host",
                    os.path.join(root, "tests", "cpp", "block_walker.cpp"), "-o", exe, f"-L{root}/dint_amd", "-ldint_hip",
                    f"-Wl,-rpath,{root}/dint_amd"], check=True)
    kind = host.SINGLE_PACKED
    for which, name in (("len", "len 1"), ("len", "len 5"), ("wide", "tail 257")):
        ix = SB.index(which, kind)
        i = ix.at[name]
        (tmp_path / "docs.dict").write_bytes(ix.docs_dict)
        (tmp_path / "freqs.dict").write_bytes(ix.freqs_dict)
        ix.index[int(ix.offsets[i]):int(ix.offsets[i + 1])].tofile(tmp_path / "list.bin")
        ix.lists[i].tofile(tmp_path / "docids.bin")
        ix.list_freqs[i].tofile(tmp_path / "freqs.bin")
        r = subprocess.run([exe, str(kind)] + [str(tmp_path / f) for f in ("docs.dict", "freqs.dict", "list.bin", "docids.bin", "freqs.bin")]
                           + ["scope"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.splitlines()[0] == "ok", f"{name}: " + r.stdout + r.stderr


# ---- 4. queries -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _norm_lens():
    """A norm_len for every docID below LEN_BOUND (any float32 values do: the models take them as given)"""
    return ((np.arange(SB.LEN_BOUND, dtype=np.int64) % 251 + 64).astype(np.float32) / np.float32(128)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _len_want():
    """(counts, scores, docids) of the 255 queries [L_n], k = 1024: ranked OR's model, checked to be ranked AND's"""
    ix = SB.index("len", host.SINGLE_PACKED)
    lists = ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds)
    out = [ranked_or.ranked_or(lists, [t], _norm_lens(), SB.LEN_BOUND, K) for t in range(255)]
    for t in range(0, 255, 9):
        a = ranked.ranked_and(lists, [t], _norm_lens(), SB.LEN_BOUND, K)
        assert a[0] == out[t][0] and np.array_equal(a[1].view(np.uint32), out[t][1].view(np.uint32)) and np.array_equal(a[2], out[t][2])
    for t, (count, _, ids) in enumerate(out):  # all n docIDs, none lost
        assert count == t + 1 and np.array_equal(np.sort(ids[:count]), ix.lists[t]) and (ids[count:] == 0xFFFFFFFF).all()
    return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


@pytest.mark.parametrize("kind", SB.KINDS)
def test_ranked_single_term_queries_return_every_posting(device, kind):
    """ranked_or_queries and ranked_and_queries with k = 1024 over [L_n], n = 1 .. 255, in one call and every seventh alone,
    under every option set of FORMS: counts n, all n docIDs in the model's order, every score bit-equal."""
    c = _on_device("len", kind)
    counts, scores, docids = _len_want()
    qi = device.QueryIndex(c.dd, c.ix.index, c.ix.offsets)
    wand = device.WandData(_norm_lens())
    qs = [[t] for t in range(255)]
    try:
        for opts in FORMS:
            with device.options(**opts):
                for run in (qi.ranked_or_queries, qi.ranked_and_queries):
                    got = run(c.fd, wand, qs, k=K)
                    bad = np.flatnonzero(got[0] != counts)
                    assert bad.size == 0, (opts, run.__name__, "counts of lengths", (bad + 1).tolist())
                    bad = np.flatnonzero((got[2] != docids).any(axis=1))
                    assert bad.size == 0, (opts, run.__name__, "docIDs of lengths", (bad + 1).tolist())
                    bad = np.flatnonzero((got[1].view(np.uint32) != scores.view(np.uint32)).any(axis=1))
                    assert bad.size == 0, (opts, run.__name__, "scores of lengths", (bad + 1).tolist())
                    for t in range(0, 255, 7):
                        one = run(c.fd, wand, [qs[t]], k=K)
                        assert int(one[0][0]) == t + 1 and np.array_equal(one[2][0], docids[t]), (opts, run.__name__, t + 1)
                        assert np.array_equal(one[1][0].view(np.uint32), scores[t].view(np.uint32)), (opts, run.__name__, t + 1)
    finally:
        qi.close()
        wand.close()


@functools.lru_cache(maxsize=None)
def _partner_want(which):
    """The queries [list, its partner] of an index and what AND / OR with freqs answer (the lists are the same under every kind)"""
    ix = SB.index(which, host.SINGLE_PACKED)
    qs = [[ix.at[name], ix.at[pname]] for name, pname in ix.partner_of.items()]
    want_and = [intersect_freqs(ix.docids, ix.freqs, ix.bounds, q) for q in qs]
    want_or = [union_freqs(ix.docids, ix.freqs, ix.bounds, q) for q in qs]
    for q, a, o in zip(qs, want_and, want_or):  # the chosen half; every near-miss counted
        n, p = int(ix.lens[q[0]]), int(ix.lens[q[1]])
        assert a[0] == (n + 1) // 2 and o[0] == n + p - a[0]
    return qs, want_and, want_or


def _exact_query_index(device, c):
    """A QueryIndex over the device buffer of `c`, handed over at c.index_bytes (device.QueryIndex pads with zeros)"""
    qi = device.QueryIndex.__new__(device.QueryIndex)
    qi.docs_dict = c.dd
    qi.blocks, qi.total = device.index_posting_lists(c.ix.index, c.ix.offsets)
    qi.n_lists = len(c.ix.offsets) - 1
    qi._index_dev = c.index_dev
    qi._h = C.c_void_p()
    device._check(device._lib.dint_query_index_create(c.dd._h, c.index_dev.data_ptr(), c.index_bytes, qi.blocks.ctypes.data,
                                                      len(qi.blocks), qi.n_lists, C.byref(qi._h)), "dint_query_index_create")
    return qi


@pytest.mark.parametrize("kind", SB.KINDS)
@pytest.mark.parametrize("which", ["wide", "edge"])
def test_and_or_queries_with_partner_lists(device, which, kind):
    """WIDE, TAIL and the draws (`wide`), EDGE (`edge`): docIDs up to 0xFFFFFFFE, out of the ranked calls' reach. Every list
    with its partner: counts and u64 freq sums of AND and OR with freqs (and the counts alone: a batch of counts is the
    workgroup-per-query form) against intersect_freqs / union_freqs, in a batch and alone, under every option set of FORMS."""
    c = _on_device(which, kind)
    qs, want_and, want_or = _partner_want(which)
    and_pairs, or_pairs = [tuple(w) for w in want_and], [tuple(w) for w in want_or]
    qi = _exact_query_index(device, c)
    try:
        for opts in FORMS:
            with device.options(**opts):
                counts, sums, _ = qi.and_queries_with_freqs(c.fd, qs)
                got = list(zip(counts.tolist(), sums.tolist()))
                bad = [c.ix.names[qs[i][0]] for i in range(len(qs)) if got[i] != and_pairs[i]]
                assert not bad, (opts, "and_freq", bad[:8])
                counts, sums, _ = qi.or_queries_with_freqs(c.fd, qs)
                got = list(zip(counts.tolist(), sums.tolist()))
                bad = [c.ix.names[qs[i][0]] for i in range(len(qs)) if got[i] != or_pairs[i]]
                assert not bad, (opts, "or_freq", bad[:8])
                assert qi.and_queries(qs).tolist() == [w[0] for w in want_and], (opts, "and")
                assert qi.or_queries(qs).tolist() == [w[0] for w in want_or], (opts, "or")
                for i, q in enumerate(qs):
                    counts, sums, _ = qi.and_queries_with_freqs(c.fd, [q])
                    assert (int(counts[0]), int(sums[0])) == and_pairs[i], (opts, "and_freq alone", c.ix.names[q[0]])
                    counts, sums, _ = qi.or_queries_with_freqs(c.fd, [q])
                    assert (int(counts[0]), int(sums[0])) == or_pairs[i], (opts, "or_freq alone", c.ix.names[q[0]])
    finally:
        qi.close()
