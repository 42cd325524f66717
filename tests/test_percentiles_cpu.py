"""Percentiles without a GPU: the two entries in the header, the library and the binding, with
DINT_ABI_VERSION still 6 and the options unchanged; the argument errors that need no device; the model (tests/percentiles.py)
against a document-at-a-time loop with sorted() on Python ints, and its invariants against the value-stats model; the
conditions that tests/test_gpu_percentiles_fuzz.py demands of its committed seeds, from the model alone; and the parser of
dint_queries' --percentiles lists (tools/percentile_list.hpp, compiled alone with g++)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import doc_values as DV
import percentiles as PC
import ranked
import value_stats as VS
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSER = os.path.join(ROOT, "tools", "percentile_list.hpp")
ENTRIES = ("dint_ranked_or_percentile_queries", "dint_ranked_and_percentile_queries")
M32 = 0xFFFFFFFF
# the entries' arguments: the filtered call's up to filter (7), then values, per_million, n_percentiles, n_queries, counts,
# matches, scores, docids, value_counts, percentile_values, stats, blocks_decoded, stream
N_ARGS = 7 + 13
OPTIONS = {"bundles", "index_concurrent", "query_lean_pages", "query_tail_pages", "query_fused_pages", "index_inline_tails", "chunk_split",
           "index_pair", "query_fused_copy", "query_batch_fused", "split_units", "refine_units"}


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "#define DINT_PERCENTILES_MAX 16u" in header and "#define DINT_PERCENTILES_MAX_RECORDS (1ull << 16)" in header
    assert device.PERCENTILES_MAX == PC.MAX_PERCENTILES == 16 and PC.MAX_RECORDS == 1 << 16
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert len(getattr(device._lib, name).argtypes) == N_ARGS == 20
        declared = header[header.index(f"int {name}("):]
        assert declared[:declared.index(";")].count(",") + 1 == N_ARGS
    assert hasattr(device.QueryIndex, "ranked_or_percentile_queries") and hasattr(device.QueryIndex, "ranked_and_percentile_queries")
    assert set(device.OPTIONS) == OPTIONS  # no new option


def test_percentiles_are_packed_or_refused_before_the_call():
    from dint_amd import device

    p = device._pack_percentiles([0, 50, 99.9, 100, 0.0001, 99.9999, 50])
    assert p.dtype == np.uint32 and p.flags["C_CONTIGUOUS"] and p.tolist() == [0, 500000, 999000, 1000000, 1, 999999, 500000]
    assert device._pack_percentiles(np.linspace(0, 100, 16)).size == 16 and device._pack_percentiles(12.5).tolist() == [125000]
    for pm in ([0], [1000000], [333333, 1, 999999], PC.sharing_a_prefix(9000, 4096), list(PC.COMMON)):
        assert device._pack_percentiles(PC.percents(pm)).tolist() == pm  # the tests' way from parts per million and back
    for bad in ([], [-0.0001], [100.0001], [50, 101], [float("nan")], [float("inf")], list(range(17))):
        with pytest.raises(ValueError):
            device._pack_percentiles(bad)


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts, matches, value_counts = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
    docids, pvalues = np.full(2048, 77, dtype=np.uint32), np.full(2048, 77, dtype=np.uint32)
    scores = np.full(2048, -1.0, dtype=np.float32)
    stats = np.full(1, 77, dtype=device._VALUE_STATS)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: everything below is refused first)
    p3 = np.array([500000, 0, 1000000], dtype=np.uint32)
    ok = dict(qi=fake, fd=fake, w=fake, k=10, cnt=counts, values=fake, pm=p3, n_p=3, vc=value_counts, pv=pvalues, st=stats)
    cases = [dict(qi=None), dict(fd=None), dict(w=None), dict(cnt=None), dict(k=0), dict(k=1025), dict(values=None), dict(pm=None),
             dict(vc=None), dict(pv=None), dict(n_p=0), dict(pm=np.zeros(17, dtype=np.uint32), n_p=17),
             dict(pm=np.array([1000001], dtype=np.uint32), n_p=1), dict(pm=np.array([0, 5, M32], dtype=np.uint32)),
             dict(n_p=1, n=(1 << 16) + 1),  # n_queries * n_percentiles past 2^16: refused before the offsets are read
             dict(pm=np.zeros(16, dtype=np.uint32), n_p=16, n=(1 << 12) + 1), dict(n_p=3, n=(1 << 16) // 3 + 1)]
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    for name in ENTRIES:
        for with_stats in (True, False):
            for change in cases:
                a = dict(ok, n=1)
                a.update(change)
                st = getattr(lib, name)(a["qi"], a["fd"], a["w"], a["k"], terms.ctypes.data, offs.ctypes.data, None, a["values"], ptr(a["pm"]),
                                        a["n_p"], a["n"], ptr(a["cnt"]), matches.ctypes.data, scores.ctypes.data, docids.ctypes.data, ptr(a["vc"]),
                                        ptr(a["pv"]), ptr(a["st"]) if with_stats else None, C.byref(blocks), None)
                assert st == -1, (name, change)
    assert counts[0] == 77 and matches[0] == 77 and value_counts[0] == 77 and blocks.value == 77
    assert stats.tobytes() == np.full(1, 77, dtype=device._VALUE_STATS).tobytes()
    assert (docids == 77).all() and (pvalues == 77).all() and (scores == -1.0).all()


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_percentiles_by_hand():
    sc = np.array([3.0, 2.0, 2.0, 1.0, 0.5, 0.25], dtype=np.float32)
    ids = np.array([0, 1, 2, 3, 4, 9], dtype=np.uint32)
    values = np.array([40, 10, 30, M32, 10, 0], dtype=np.uint32)  # (document 9 is past the column: no value)
    n, out = PC.percentiles((sc, ids), None, values, [0, 1000000, 500000, 250000, 249999, 999999, 750000])
    # the sort: 10 10 30 40 M32; the ranks (4 * p) // 1000000 = 0 4 2 1 0 3 3
    assert n == 5 and out.dtype == np.uint32 and out.tolist() == [10, M32, 30, 10, 10, 40, 40]
    assert [PC.rank_of(2, p) for p in (0, 499999, 500000, 999999, 1000000)] == [0, 0, 0, 0, 1]  # two values: the LOWER median
    assert PC.rank_of(1, 1000000) == 0 and PC.rank_of((1 << 32) - 1, 1000000) == (1 << 32) - 2  # (the product needs 64 bits)
    mask = np.array([False] * 9 + [True])
    assert PC.percentiles((sc, ids), mask, values, [0, 500000])[0] == 0 and not PC.percentiles((sc, ids), mask, values, [0, 500000])[1].any()
    nothing = (np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint32))
    assert PC.percentiles(nothing, None, values, [7])[0] == 0 and PC.percentiles(nothing, None, values, [7])[1].tolist() == [0]
    one = PC.percentiles((sc[:1], ids[:1]), None, values, [0, 500000, 1000000])
    assert one[0] == 1 and one[1].tolist() == [40, 40, 40]
    counts, stacked = PC.stacked([PC.percentiles((sc, ids), None, values, [0, 1000000]), PC.percentiles(nothing, None, values, [0, 1000000])], 2)
    assert counts.dtype == np.uint64 and counts.tolist() == [5, 0] and stacked.tolist() == [[10, M32], [0, 0]]
    assert PC.stacked([], 3)[1].shape == (0, 3)


def test_the_named_columns_and_sets_are_what_they_are_said_to_be():
    top = 9000
    cols = PC.named_columns(top)
    assert set(cols) == {"all equal", "zeros", "ones", "v = d", "reverse", "top byte", "lowest byte", "two halves", "wide", "half", "empty"}
    assert np.unique(cols["all equal"]).size == 1 and not cols["zeros"].any() and (cols["ones"] == M32).all()
    assert (np.diff(cols["v = d"].astype(np.int64)) == 1).all() and (np.diff(cols["reverse"].astype(np.int64)) == -1).all()
    assert np.unique(cols["top byte"] >> 24).size == 256 and np.unique(cols["top byte"] & 0xFFFFFF).size == 1
    assert np.unique(cols["lowest byte"] >> 8).size == 1 and np.unique(cols["lowest byte"] & 0xFF).size == 251
    lo, hi = np.unique(cols["two halves"]).tolist()
    assert hi == lo + 1 and all((lo >> s) & 0xFF != (hi >> s) & 0xFF for s in (0, 8, 16, 24))  # a boundary of a bin in every round
    assert (cols["two halves"] == lo).sum() == (cols["two halves"] == hi).sum() == top // 2
    assert cols["half"].size == top // 2 and cols["empty"].size == 0 and np.unique(cols["wide"] >> 24).size == 256
    sets = PC.percentile_sets(top)
    assert [len(sets[n]) for n in ("the minimum", "the maximum", "the median", "both ends")] == [1, 1, 1, 2]
    d = sets["descending, one twice"]
    assert d == sorted(d, reverse=True) and len(set(d)) == len(d) - 1
    every = (np.ones(top, dtype=np.float32), np.arange(top, dtype=np.uint32))
    spread = PC.percentiles(every, None, cols["top byte"], sets["sixteen, spread"])[1]
    assert spread.size == 16 and np.unique(spread >> 24).size == 16  # sixteen different top bytes
    near = PC.percentiles(every, None, cols["v = d"], sets["sixteen, one prefix"])[1]
    assert near.tolist() == list(range(4096, 4112)) and np.unique(near >> 8).size == 1  # one prefix down to the last byte
    # the median of the two halves, matched whole: the last of the lower half
    assert PC.percentiles(every, None, cols["two halves"], [500000, 500112])[1].tolist() == [lo, hi]


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_per_document_loop(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 4, x.size).astype(np.uint32) for x in lists]
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = np.ones(num_docs, dtype=np.float32) if seed % 2 else ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    bl = ranked.BuilderLists(docids, fr, bounds)
    columns = dict(PC.named_columns(num_docs, seed=seed))
    columns["drawn"] = DV.fuzz_values(r, num_docs)[1]
    if seed in (3, 4):
        columns["drawn"] = columns["drawn"][:num_docs // 3]  # a column shorter than the index
    sets = dict(PC.percentile_sets(num_docs))
    sets["sixteen, one prefix"] = PC.sharing_a_prefix(num_docs, min(16, num_docs - 17))
    sets["drawn"] = PC.draw_percentiles(seed)
    sets["drawn, every third"] = PC.draw_percentiles(3 * seed)
    asked = valued = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], []):
            every = VS.DF.every_match(bl, q, nl, num_docs, conjunctive)
            for n_mask in (None, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                for cname, values in columns.items():
                    stats = VS.value_stats(every, mask, values, None, 1)[0]
                    for sname, pm in sets.items():
                        n, out = PC.percentiles(every, mask, values, pm)
                        n2, out2 = PC.percentiles_by_loop(every, mask, values, pm)
                        assert n == n2 and out.dtype == out2.dtype and out.tobytes() == out2.tobytes(), (cname, sname, q)
                        assert n == stats[0]
                        order = np.argsort(pm, kind="stable")
                        assert (np.diff(out[order].astype(np.int64)) >= 0).all()  # non-decreasing in per_million
                        for p, v in zip(pm, out.tolist()):
                            if n and p == 0:
                                assert v == stats[2]  # the minimum of the value-stats model
                            if n and p == 1000000:
                                assert v == stats[3]  # ... and the maximum
                            assert n or v == 0
                        asked, valued = asked + len(pm), valued + n
    assert asked > 1000 and valued > 1000
    assert PC.draw_percentiles(3 * seed)[:2] == [0, 1000000]


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_draws_meet_their_conditions():
    """tests/test_gpu_percentiles_fuzz.py states four conditions on its cases (check_shares there). They are properties of the
    committed seeds and the draws: replayed here from the model, so that they are settled without a device, with the figures of
    that file."""
    import test_gpu_percentiles_fuzz as P

    totals, sizes, forced = [], set(), 0
    for seed, kind, ds, fs in P.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = P.Z.F.make_dictionary(r, kind, **ds), P.Z.F.make_dictionary(r, kind, **fs)
        for i in range(P.CASES_PER_DICTIONARY):
            case = P.Y.draw_collapse_case(Dd, Df, 100 * seed + i)
            totals.append(P.model_shares(case))
            pm = P.draws_of(case)[2]
            sizes.add(len(pm))
            assert 1 <= len(pm) <= 16 and all(0 <= p <= 1000000 for p in pm)
            if case.base.seed % 3 == 0:
                forced += 1
                assert pm[:2] == [0, 1000000]
    assert len(totals) == 240 and sizes == set(range(1, 17)) and forced >= 240 // 3 - 6  # every size is drawn
    P.check_shares(np.sum(totals, axis=0))
    assert [tuple(t) for t in np.sum(totals, axis=0).tolist()] == [P.FIGURES["or"], P.FIGURES["and"]]


# ---- the --percentiles parser -------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <string>
#include "%s"
int main(int argc, char** argv) {
    try {
        const std::vector<uint32_t> p = tool::parse_percentiles(argc > 1 ? argv[1] : "");
        std::printf("%%zu", p.size());
        for (uint32_t v : p) std::printf(" %%u", v);
        std::printf("\n");
    } catch (std::exception const& e) {
        std::printf("error %%s\n", e.what());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def parser_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the percentiles parser"
    tmp = tmp_path_factory.mktemp("percentile_list")
    src, exe = os.path.join(tmp, "parse.cpp"), os.path.join(tmp, "parse")
    with open(src, "w") as f:
        f.write(PROGRAM % PARSER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    return exe


def _parse(exe, text):
    """-> parts per million as a list, or None for a refused list"""
    out = subprocess.run([exe, text], check=True, capture_output=True, text=True).stdout.split()
    if out[0] == "error":
        return None
    assert len(out) == int(out[0]) + 1
    return [int(x) for x in out[1:]]


def test_percentile_lists(parser_exe):
    assert _parse(parser_exe, "0") == [0] and _parse(parser_exe, "100") == [1000000] and _parse(parser_exe, "99.9999") == [999999]
    assert _parse(parser_exe, "50,50") == [500000, 500000] and _parse(parser_exe, "50,90,99.9") == [500000, 900000, 999000]
    assert _parse(parser_exe, "0.0001,100.0000,007.5,0.0") == [1, 1000000, 75000, 0] and _parse(parser_exe, "99,1") == [990000, 10000]
    assert _parse(parser_exe, "0000100") == [1000000] and _parse(parser_exe, "12.3456") == [123456]
    most = ",".join(str(i) for i in range(16))
    assert _parse(parser_exe, most) == [10000 * i for i in range(16)]
    for bad in ("100.0001", "1.23456", "", most + ",16", ",", "1,", ",1", "1,,2", "-1", "+1", "1e1", "0x10", "1 ,2", "1, 2", "1;2", "a", ".5", "5.",
                "1.2.3", "101", "1000", "4294967297", "0001000", "99999999999999999999"):
        assert _parse(parser_exe, bad) is None, bad
