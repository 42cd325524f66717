"""Value statistics without a GPU: the two entries in the header, the library and the binding, with
DINT_ABI_VERSION still 6; the argument errors that need no device; the model (tests/value_stats.py) against a
document-at-a-time loop on Python ints; the conditions that tests/test_gpu_value_stats_fuzz.py demands of its committed seeds,
from the model alone; and the parser of dint_queries' --edges lists (tools/value_edges.hpp, compiled alone with g++)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import doc_values as DV
import ranked
import value_stats as VS
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSER = os.path.join(ROOT, "tools", "value_edges.hpp")
ENTRIES = ("dint_ranked_or_value_stats_queries", "dint_ranked_and_value_stats_queries")
M32 = 0xFFFFFFFF
# the entries' arguments: the filtered call's up to filter (7), then values, edges, n_edges, n_queries, counts, matches, scores,
# docids, stats, bucket_counts, hit_values, blocks_decoded, stream
N_ARGS = 7 + 13


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "#define DINT_VALUE_STATS_MAX_EDGES 1023u" in header and "typedef struct dint_value_stats" in header
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert len(getattr(device._lib, name).argtypes) == N_ARGS
        declared = header[header.index(f"int {name}("):]
        assert declared[:declared.index(";")].count(",") + 1 == N_ARGS
        assert hasattr(device.QueryIndex, name[len("dint_"):])
    # dint_value_stats {uint64_t n; uint64_t sum; uint32_t min; uint32_t max;}: 24 bytes
    assert device._VALUE_STATS.itemsize == 24
    assert [device._VALUE_STATS.fields[n][1] for n in ("n", "sum", "min", "max")] == [0, 8, 16, 20]
    assert device._VALUE_STATS == VS.STATS_DTYPE and device.VALUE_STATS_MAX_EDGES == VS.MAX_EDGES == 1023


def test_edges_are_packed_or_refused_before_the_call():
    from dint_amd import device

    assert device._pack_value_edges(None).size == 0 and device._pack_value_edges([]).size == 0
    e = device._pack_value_edges([0, 5, M32])
    assert e.dtype == np.uint32 and e.tolist() == [0, 5, M32] and e.flags["C_CONTIGUOUS"]
    assert device._pack_value_edges(np.arange(1023)).size == 1023
    for bad in ([5, 5], [7, 3], [-1, 4], [0, 1 << 32], list(range(1024))):
        with pytest.raises(ValueError):
            device._pack_value_edges(bad)


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts, matches = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
    docids, hit_values = np.full(2048, 77, dtype=np.uint32), np.full(2048, 77, dtype=np.uint32)
    scores = np.full(2048, -1.0, dtype=np.float32)
    stats = np.full(1, 77, dtype=device._VALUE_STATS)
    buckets = np.full(2048, 77, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: everything below is refused first)
    e3 = np.array([1, 5, 9], dtype=np.uint32)
    many = np.arange(1024, dtype=np.uint32)
    ok = dict(qi=fake, fd=fake, w=fake, k=10, cnt=counts, values=fake, edges=e3, n_edges=3, st=stats, rows=buckets)
    cases = [dict(qi=None), dict(fd=None), dict(w=None), dict(cnt=None), dict(k=0), dict(k=1025), dict(values=None), dict(st=None),
             dict(edges=many, n_edges=1024), dict(edges=None), dict(rows=None), dict(edges=np.array([5, 5], dtype=np.uint32), n_edges=2),
             dict(edges=np.array([7, 3], dtype=np.uint32), n_edges=2), dict(edges=np.array([1, 2, 2], dtype=np.uint32)),
             dict(n_edges=1023, n=(1 << 18) + 1, edges=many)]  # n_queries * (n_edges + 1) past 2^28: refused before the offsets are read
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    for name in ENTRIES:
        for change in cases:
            a = dict(ok, n=1)
            a.update(change)
            assert getattr(lib, name)(a["qi"], a["fd"], a["w"], a["k"], terms.ctypes.data, offs.ctypes.data, None, a["values"], ptr(a["edges"]),
                                      a["n_edges"], a["n"], ptr(a["cnt"]), matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                                      ptr(a["st"]), ptr(a["rows"]), hit_values.ctypes.data, C.byref(blocks), None) == -1, (name, change)
    assert counts[0] == 77 and matches[0] == 77 and blocks.value == 77 and stats.tobytes() == np.full(1, 77, dtype=device._VALUE_STATS).tobytes()
    assert (docids == 77).all() and (hit_values == 77).all() and (scores == -1.0).all() and (buckets == 77).all()


# ---- the model ----------------------------------------------------------------------------------------------------------
def _same(x, y):
    assert x[0] == y[0], (x[0], y[0])
    for a, b in zip(x[1:], y[1:]):
        assert (a is None and b is None) or (a.dtype == b.dtype and a.tobytes() == b.tobytes())


def test_buckets_by_hand():
    sc = np.array([3.0, 2.0, 2.0, 1.0, 0.5], dtype=np.float32)
    ids = np.array([0, 1, 2, 3, 9], dtype=np.uint32)
    values = np.array([4, 5, 6, M32, 0, 0], dtype=np.uint32)  # (document 9 is past the column: no value)
    stats, row, hv = VS.value_stats((sc, ids), None, values, [5, 6], 3)
    assert stats == (4, 4 + 5 + 6 + M32, 4, M32) and row.tolist() == [1, 1, 2] and hv.tolist() == [4, 5, 6]
    # an edge equal to a value: the value is in the bucket that BEGINS there; edges at both ends
    assert VS.value_stats((sc, ids), None, values, [0, M32], 5)[1].tolist() == [0, 3, 1]
    assert VS.value_stats((sc, ids), None, values, [0], 5)[1].tolist() == [0, 4] and VS.value_stats((sc, ids), None, values, [M32], 5)[1].tolist() == [3, 1]
    assert VS.value_stats((sc, ids), None, values, [], 5)[1] is None and VS.value_stats((sc, ids), None, values, None, 5)[1] is None
    # a hit past the column: value 0 among the hits, and it counts nowhere
    assert VS.value_stats((sc, ids), None, values, [5], 5)[2].tolist() == [4, 5, 6, M32, 0]
    mask = np.array([False] * 9 + [True])
    stats, row, hv = VS.value_stats((sc, ids), mask, values, [5], 2)
    assert stats == VS.EMPTY == (0, 0, M32, 0) and row.tolist() == [0, 0] and hv.tolist() == [0, 0]
    nothing = (np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint32))
    assert VS.value_stats(nothing, None, values, [5], 2)[0] == VS.EMPTY
    out = VS.stacked([VS.value_stats((sc, ids), None, values, [5, 6], 3), VS.value_stats(nothing, None, values, [5, 6], 3)], 3, 2)
    assert out[0].dtype.itemsize == 24 and out[0]["n"].tolist() == [4, 0] and out[0]["min"].tolist() == [4, M32] and out[1].shape == (2, 3)
    assert VS.stacked([], 3, 0)[1] is None and VS.stacked([], 3, 2)[1].shape == (0, 3)


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
    kind, values, _ = DV.fuzz_values(r, num_docs)
    if seed in (3, 4):
        values = values[:num_docs // 3]  # a column shorter than the index
    sets = VS.edge_sets(values)
    assert [len(sets[n]) for n in ("none", "0", "the top", "both ends", "a present value", "1023")] == [0, 1, 1, 2, 1, 1023]
    assert sets["a present value"][0] in values.tolist()
    sets["drawn"] = VS.fuzz_edges(r, values)[1].tolist()
    past = valued = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], []):
            every = VS.DF.every_match(bl, q, nl, num_docs, conjunctive)
            for n_mask in (None, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                ids = VS.matches_in(every, mask)[1]
                for name, edges in sets.items():
                    for k in (1, 10):
                        got = VS.value_stats(every, mask, values, edges, k)
                        _same(got, VS.value_stats_by_loop(every, mask, values, edges, k))
                        (n, total, lo, hi), row, hv = got
                        assert (row is None) == (len(edges) == 0) and (row is None or int(row.sum()) == n), (name, q)
                        assert ids.size - n == int((ids >= len(values)).sum())  # matches - n: the matches past the column
                        assert (n == 0 and got[0] == VS.EMPTY) or (lo <= hi and n * lo <= total <= n * hi)
                past, valued = past + ids.size - n, valued + n
    assert valued > 100 and (past > 20) == (seed in (3, 4))


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_draws_meet_their_conditions():
    """tests/test_gpu_value_stats_fuzz.py states four conditions on its cases (check_shares there). They are properties of the
    committed seeds and the draws: replayed here from the model, so that they are settled without a device, with the figures of
    that file."""
    import test_gpu_value_stats_fuzz as P

    totals, counts = [], {}
    for seed, kind, ds, fs in P.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = P.Z.F.make_dictionary(r, kind, **ds), P.Z.F.make_dictionary(r, kind, **fs)
        for i in range(P.CASES_PER_DICTIONARY):
            case = P.Y.draw_collapse_case(Dd, Df, 100 * seed + i)
            totals.append(P.model_shares(case))
            which = P.draws_of(case)[2]
            counts[which] = counts.get(which, 0) + 1
    assert len(totals) == 240 and set(counts) == set(VS.EDGE_COUNTS) and min(counts.values()) >= 10  # every edge count is drawn
    P.check_shares(np.sum(totals, axis=0))
    assert [tuple(t) for t in np.sum(totals, axis=0).tolist()] == [P.FIGURES["or"], P.FIGURES["and"]]


# ---- the --edges parser -------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <string>
#include "%s"
int main(int argc, char** argv) {
    try {
        const std::vector<uint32_t> e = tool::parse_value_edges(argc > 1 ? argv[1] : "");
        std::printf("%%zu", e.size());
        for (uint32_t v : e) std::printf(" %%u", v);
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
    assert cxx, "g++ is needed to compile the edges parser"
    tmp = tmp_path_factory.mktemp("value_edges")
    src, exe = os.path.join(tmp, "parse.cpp"), os.path.join(tmp, "parse")
    with open(src, "w") as f:
        f.write(PROGRAM % PARSER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    return exe


def _parse(exe, text):
    """-> the edges as a list, or None for a refused list"""
    out = subprocess.run([exe, text], check=True, capture_output=True, text=True).stdout.split()
    if out[0] == "error":
        return None
    assert len(out) == int(out[0]) + 1
    return [int(x) for x in out[1:]]


def test_edges_lists(parser_exe):
    assert _parse(parser_exe, "10,50,200") == [10, 50, 200] and _parse(parser_exe, "0") == [0] and _parse(parser_exe, "4294967295") == [M32]
    assert _parse(parser_exe, "0,4294967295") == [0, M32] and _parse(parser_exe, "007,8") == [7, 8]
    most = ",".join(str(3 * i) for i in range(1023))
    assert _parse(parser_exe, most) == [3 * i for i in range(1023)]
    for bad in ("", ",", "1,", ",1", "1,,2", "-1", "+1", "1,-2", "0x10", "1 ,2", "1, 2", "1;2", "a", "4294967296", "99999999999", "5,5", "7,3", "1,2,2",
                most + ",4000"):
        assert _parse(parser_exe, bad) is None, bad
