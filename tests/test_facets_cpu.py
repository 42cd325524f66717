"""Faceted ranked queries without a GPU: the entries in the header, the library and the binding, with
DINT_ABI_VERSION still 6; the argument errors that need no device; the model (tests/facets.py) against a per-document loop;
the binding's input forms; the parser of dint_queries' --facets files (tools/doc_facets_file.hpp, compiled alone with g++);
and the shares that tests/test_gpu_facets_fuzz.py demands of its committed seeds, from the model alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import facets as FA
import ranked
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSER = os.path.join(ROOT, "tools", "doc_facets_file.hpp")
HANDLE = ("dint_doc_facets_create", "dint_doc_facets_info_get", "dint_doc_facets_group_sizes", "dint_doc_facets_destroy")
ENTRIES = ("dint_ranked_or_faceted_queries", "dint_ranked_and_faceted_queries")


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "typedef struct dint_doc_facets dint_doc_facets;" in header and "} dint_doc_facets_info;" in header
    assert "#define DINT_FACET_NONE 0xFFFFFFFFu" in header and "#define DINT_FACETS_MAX_GROUPS 65536u" in header
    assert "4 BYTES PER DOCUMENT" in header  # (the handle's device memory is stated)
    for name in HANDLE + ENTRIES:
        assert f" {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
    for name in ENTRIES:
        assert hasattr(device.QueryIndex, name[len("dint_"):])
    assert [f[0] for f in device.DocFacetsInfo._fields_] == ["num_docs", "n_groups", "n_grouped"]
    assert device.FACET_NONE == 0xFFFFFFFF and device.FACETS_MAX_GROUPS == 65536 and hasattr(device.DocFacets, "close")


def test_argument_errors_need_no_device():
    import ctypes as C

    from dint_amd import device

    lib = device._lib
    h = C.c_void_p(77)
    word = np.zeros(4, dtype=np.uint32)
    # refused before any device is asked for: no groups, too many, too many documents, a null map with documents, a null out
    assert lib.dint_doc_facets_create(0, word.ctypes.data, 4, 0, C.byref(h)) == -1 and h.value is None
    h = C.c_void_p(77)
    assert lib.dint_doc_facets_create(0, word.ctypes.data, 4, 65537, C.byref(h)) == -1 and h.value is None
    assert lib.dint_doc_facets_create(0, word.ctypes.data, 1 << 32, 4, C.byref(h)) == -1
    assert lib.dint_doc_facets_create(0, None, 4, 4, C.byref(h)) == -1
    assert lib.dint_doc_facets_create(0, word.ctypes.data, 4, 4, None) == -1
    assert lib.dint_doc_facets_info_get(None, C.byref(device.DocFacetsInfo())) == -1
    assert lib.dint_doc_facets_group_sizes(None, word.ctypes.data) == -1
    lib.dint_doc_facets_destroy(None)
    # the calls: the filtered entries' own refusals come first, and nothing is written
    counts = np.full(1, 77, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    rows = np.full(8, 77, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for name in ENTRIES:
        call = getattr(lib, name)
        for qi, fd, w, k, cnt in ((None, fake, fake, 10, counts), (fake, None, fake, 10, counts), (fake, fake, None, 10, counts),
                                  (fake, fake, fake, 0, counts), (fake, fake, fake, 1025, counts), (fake, fake, fake, 10, None)):
            for facets in (None, fake):
                assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, facets, 1, cnt.ctypes.data if cnt is not None else None,
                            None, scores.ctypes.data, None, rows.ctypes.data, C.byref(blocks), None) == -1
                assert counts[0] == 77 and blocks.value == 77 and not scores.any() and (rows == 77).all()  # nothing is written


def test_the_binding_takes_any_integers_negatives_and_none():
    from dint_amd import device

    N = device.FACET_NONE
    m, n = device.doc_facets_map([0, 2, -1, None, 1])
    assert m.dtype == np.uint32 and m.tolist() == [0, 2, N, N, 1] and n == 3
    for dtype in (np.int8, np.int16, np.int32, np.int64):
        m, n = device.doc_facets_map(np.array([3, -1, 0, -5], dtype=dtype))
        assert m.tolist() == [3, N, 0, N] and n == 4
    for dtype in (np.uint8, np.uint16, np.uint32, np.uint64):
        m, n = device.doc_facets_map(np.array([3, 0, 7], dtype=dtype), 9)
        assert m.dtype == np.uint32 and m.tolist() == [3, 0, 7] and n == 9
    m, n = device.doc_facets_map(np.array([N, 5], dtype=np.uint32))  # (NONE itself, as the C ABI has it)
    assert m.tolist() == [N, 5] and n == 6
    assert device.doc_facets_map([])[1] == 1 and device.doc_facets_map([-1, None])[1] == 1 and device.doc_facets_map([])[0].size == 0
    assert device.doc_facets_map([[0, 1], [2, -1]])[0].tolist() == [0, 1, 2, N]  # (any shape: flattened)
    m, n = device.doc_facets_map([70000], 3)  # (passed on: the library refuses it)
    assert m.tolist() == [70000] and n == 3
    with pytest.raises(TypeError):
        device.doc_facets_map([0.5, 1.0])
    with pytest.raises(ValueError):
        device.doc_facets_map([1 << 32])
    for name in FA.MAPS:  # the model's maps go through unchanged but for NONE
        g = FA.named_map(name, 300, 7)
        m, n = device.doc_facets_map(g, 7)
        assert np.array_equal(m.astype(np.int64), np.where(g == FA.NONE, N, g))


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_the_named_maps_are_what_they_are_said_to_be():
    for num_docs, n_groups in ((1, 1), (257, 8), (9000, 255), (9000, 257), (1000, 4096)):
        for name in FA.MAPS:
            g = FA.named_map(name, num_docs, n_groups)
            assert g.dtype == np.int64 and g.size == num_docs and ((g == FA.NONE) | ((g >= 0) & (g < n_groups))).all(), name
        c = FA.named_map("clustered", num_docs, n_groups)
        assert (np.diff(c) >= 0).all() and c[0] == 0  # consecutive runs
        assert FA.named_map("striped", num_docs, n_groups)[:min(num_docs, n_groups)].tolist() == list(range(min(num_docs, n_groups)))
        assert set(FA.named_map("one group", num_docs, n_groups).tolist()) == {n_groups - 1}
        assert set(FA.named_map("none", num_docs, n_groups).tolist()) == {FA.NONE}
        e = FA.named_map("every other document NONE", num_docs, n_groups)
        assert (e[1::2] == FA.NONE).all() and np.array_equal(e[::2], c[::2])


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_per_document_loop(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 6, x.size).astype(np.uint32) for x in lists]
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    bl = ranked.BuilderLists(docids, fr, bounds)
    counted = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], [2, 0], []):
            sets = [set(lists[t].tolist()) for t in q]
            docs = (set.intersection(*sets) if conjunctive else set.union(*sets)) if sets else set()
            every = FA.every_match(bl, q, nl, num_docs, conjunctive)
            assert set(every[1].tolist()) == docs
            for n_mask in (None, num_docs, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                ids = FA.matches_in(every, mask)
                assert sorted(ids.tolist()) == sorted(d for d in docs if mask is None or (d < n_mask and mask[d]))
                for name in FA.MAPS:
                    for n_map, n_groups in ((num_docs, 3), (num_docs // 2, 17), (num_docs + 9, 300)):  # the map: at, below, above
                        g = FA.named_map(name, n_map, n_groups, seed=seed)
                        row, none = FA.row_of(g, n_groups, ids)
                        by_loop, none_by_loop = FA.row_by_loop(g, n_groups, ids)
                        assert row.dtype == np.uint32 and row.size == n_groups
                        assert np.array_equal(row, by_loop) and none == none_by_loop
                        assert int(row.sum()) + none == ids.size  # the row's sum plus the matches in no group: the matches
                        if n_map < num_docs:
                            assert none >= int((ids >= n_map).sum())
                        counted += int(row.sum())
    assert counted > 1000
    g = FA.named_map("every other document NONE", 100, 5)
    assert FA.sizes_of(g, 5)[0].tolist() == [10] * 5 and FA.sizes_of(g, 5)[1] == 50
    assert FA.sizes_of(np.zeros(0, dtype=np.int64), 3)[0].tolist() == [0, 0, 0]


# ---- the --facets file parser -------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include "%s"
int main() {
    try {
        const tool::doc_facets_map f = tool::parse_doc_facets(std::cin);
        std::printf("%%llu %%u %%zu", (unsigned long long)f.num_docs, f.n_groups, f.group_of.size());
        for (uint32_t g : f.group_of) std::printf(" %%u", g);
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
    assert cxx, "g++ is needed to compile the facets file parser"
    tmp = tmp_path_factory.mktemp("doc_facets_file")
    src, exe = os.path.join(tmp, "parse.cpp"), os.path.join(tmp, "parse")
    with open(src, "w") as f:
        f.write(PROGRAM % PARSER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    return exe


def _parse(exe, text):
    """-> (num_docs, n_groups, {document: group} of the documents in a group), or None for a refused file"""
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    if out[0] == "error":
        return None
    num_docs, n_groups, n = int(out[0]), int(out[1]), int(out[2])
    g = [int(x) for x in out[3:]]
    assert len(g) == n == num_docs
    return num_docs, n_groups, {d: x for d, x in enumerate(g) if x != 0xFFFFFFFF}


def test_facets_files(parser_exe):
    assert _parse(parser_exe, "") == (0, 1, {})
    assert _parse(parser_exe, "\n  \n") == (0, 1, {})
    assert _parse(parser_exe, "5 0\n") == (6, 1, {5: 0})
    assert _parse(parser_exe, "5 3\n") == (6, 4, {5: 3})
    assert _parse(parser_exe, "3:7 2\n") == (7, 3, {3: 2, 4: 2, 5: 2, 6: 2})
    assert _parse(parser_exe, "  3:5   1  \r\n\n10\t4\n") == (11, 5, {3: 1, 4: 1, 10: 4})
    assert _parse(parser_exe, "7:7 9\n9:3 1\n") == (0, 10, {})                 # empty and inverted intervals name no document
    assert _parse(parser_exe, "0:10 1\n4 2\n") == (10, 3, {**{d: 1 for d in range(10)}, 4: 2})  # later lines win
    assert _parse(parser_exe, "4 2\n0:10 1\n") == (10, 3, {d: 1 for d in range(10)})
    assert _parse(parser_exe, "0:10 1\n2:5 0\n3 7\n") == (10, 8, {**{d: 1 for d in range(10)}, 2: 0, 3: 7, 4: 0})
    assert _parse(parser_exe, "100 65535\n")[1] == 65536
    r = np.random.default_rng(6)
    lines, want = [], {}
    for _ in range(200):
        lo, g = int(r.integers(0, 5000)), int(r.integers(0, 40))
        if r.random() < 0.5:
            lines.append(f"{lo} {g}")
            want[lo] = g
        else:
            hi = lo + int(r.integers(-3, 200))
            lines.append(f"{lo}:{hi} {g}")
            want.update({d: g for d in range(lo, hi)})
    got = _parse(parser_exe, "\n".join(lines))
    assert got[0] == max(want) + 1 and got[2] == want and got[1] <= 40
    for bad in ("x 1\n", "1\n", "1 2 3\n", "1:2:3 0\n", ":5 0\n", "5: 0\n", "-1 0\n", "1 -1\n", "4294967295 0\n", "0:4294967296 0\n",
                "1.5 0\n", "1 65536\n", "1 x\n"):
        assert _parse(parser_exe, bad) is None, bad
    # the top of the range, without a map of it: an empty interval there names no document
    assert _parse(parser_exe, "4294967295:4294967295 1\n4294967294:4294967290 0\n7 0\n") == (8, 2, {7: 0})


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_seeds_meet_their_conditions():
    """tests/test_gpu_facets_fuzz.py asserts, on the device's own outputs, that at least half of its (case, query) pairs match
    something and that at least half have their matches in at least two groups, for either entry (check_shares there). These
    are properties of the committed seeds: replayed here from the model, so that they are settled without a device. Both
    forms of the counting kernel and both kinds of call are among the cases."""
    import test_gpu_facets_fuzz as Y

    totals, lds_form, with_filter, kinds, past_the_map = [], 0, 0, set(), 0
    for seed, kind, ds, fs in Y.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = Y.Z.F.make_dictionary(r, kind, **ds), Y.Z.F.make_dictionary(r, kind, **fs)
        for i in range(Y.CASES_PER_DICTIONARY):
            case = Y.draw_facet_case(Dd, Df, 100 * seed + i)
            totals.append(Y.model_shares(case))
            lds_form += case.n_groups <= 256
            with_filter += case.mask is not None
            past_the_map += len(case.group_of) < case.base.num_docs
            kinds.add(case.map_kind)
            assert 1 <= case.n_groups <= 600
    n = len(totals)
    assert n == 240 and kinds == set(FA.MAPS)
    assert n // 3 < lds_form < 2 * n // 3 and n // 3 < with_filter < 2 * n // 3 and past_the_map > n // 10
    Y.check_shares(np.sum(totals, axis=0))
    assert np.sum(totals, axis=0).tolist() == [[4800, 4577, 3689], [4800, 3656, 2559]]  # (the figures of that file's docstring)
