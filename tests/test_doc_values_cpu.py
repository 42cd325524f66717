"""Document values without a GPU: the entries in the header, the library and the binding, with
DINT_ABI_VERSION still 6; the argument errors that need no device; the float mapping; the model (tests/doc_values.py) against a
document-at-a-time loop on the 64-bit integer keys; and the conditions that tests/test_gpu_doc_values_fuzz.py demands of its
committed seeds, from the model alone; and the parser of dint_queries' --values files (tools/doc_values_file.hpp, compiled
alone with g++)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import doc_values as DV
import ranked
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARSER = os.path.join(ROOT, "tools", "doc_values_file.hpp")
SORTED = ("dint_ranked_or_sorted_queries", "dint_ranked_and_sorted_queries")
M32 = 0xFFFFFFFF


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "typedef struct dint_value_cursor" in header and "#define DINT_SORT_DESC 0u" in header and "#define DINT_SORT_ASC 1u" in header
    for name, n_args in (("dint_doc_values_create", 4), ("dint_doc_values_info_get", 2), ("dint_doc_values_destroy", 1),
                         ("dint_doc_filter_create_from_values", 5), (SORTED[0], 19), (SORTED[1], 19)):
        assert f" {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert len(getattr(device._lib, name).argtypes) == n_args
    for name in SORTED:
        assert hasattr(device.QueryIndex, name[len("dint_"):])
    assert hasattr(device.QueryIndex, "doc_filter_from_values") and hasattr(device.QueryIndex, "ranked_pages")
    assert hasattr(device.DocValues, "from_float32") and hasattr(device.DocValues, "close")
    assert (device.SORT_DESC, device.SORT_ASC) == (0, 1)
    # dint_value_cursor {uint32_t value; uint32_t docid; uint32_t set;}: 12 bytes
    assert device._VALUE_CURSOR.itemsize == 12
    assert [device._VALUE_CURSOR.fields[n][1] for n in ("value", "docid", "set")] == [0, 4, 8]


def test_cursors_are_packed_as_the_struct():
    from dint_amd import device

    assert device._pack_value_cursors(None, 3) is None
    c = device._pack_value_cursors([None, (M32, 7), (0, M32)], 3)
    assert c["set"].tolist() == [0, 1, 1] and c["value"].tolist() == [0, M32, 0] and c["docid"].tolist() == [0, 7, M32]
    assert c.tobytes()[12:24] == np.array([M32, 7, 1], dtype="<u4").tobytes()
    with pytest.raises(ValueError):
        device._pack_value_cursors([(1 << 32, 0)], 1)
    with pytest.raises(ValueError):
        device._pack_value_cursors([None], 2)


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts, matches, skipped = (np.full(1, 77, dtype=np.uint64) for _ in range(3))
    hit_values, docids = np.full(2048, 77, dtype=np.uint32), np.full(2048, 77, dtype=np.uint32)
    scores = np.full(2048, -1.0, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    cursor = np.array([(1, 3, 1)], dtype=device._VALUE_CURSOR)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for qi, fd, w, k, cnt, ids in ((None, fake, fake, 10, counts, docids), (fake, None, fake, 10, counts, docids),
                                   (fake, fake, None, 10, counts, docids), (fake, fake, fake, 0, counts, docids),
                                   (fake, fake, fake, 1025, counts, docids), (fake, fake, fake, 10, None, docids)):
        for after in (None, cursor.ctypes.data):
            for name in SORTED:
                for values in (None, fake):
                    for order in (0, 1, 2):
                        assert getattr(lib, name)(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, values, order, after, 1,
                                                  cnt.ctypes.data if cnt is not None else None, matches.ctypes.data, skipped.ctypes.data,
                                                  hit_values.ctypes.data, ids.ctypes.data, scores.ctypes.data, C.byref(blocks), None) == -1
    assert counts[0] == 77 and matches[0] == 77 and skipped[0] == 77 and blocks.value == 77
    assert (hit_values == 77).all() and (docids == 77).all() and (scores == -1.0).all()
    # the handle and the value-range filter
    h = C.c_void_p(77)
    v = np.zeros(4, dtype=np.uint32)
    assert lib.dint_doc_values_create(0, v.ctypes.data, 4, None) == -1
    assert lib.dint_doc_values_create(0, v.ctypes.data, 1 << 32, C.byref(h)) == -1 and h.value is None
    h = C.c_void_p(77)
    assert lib.dint_doc_values_create(0, None, 4, C.byref(h)) == -1 and h.value is None
    info = device.DocValuesInfo()
    assert lib.dint_doc_values_info_get(None, C.byref(info)) == -1 and lib.dint_doc_values_info_get(fake, None) == -1
    lib.dint_doc_values_destroy(None)
    h = C.c_void_p(77)
    assert lib.dint_doc_filter_create_from_values(None, fake, 0, 1, C.byref(h)) == -1
    assert lib.dint_doc_filter_create_from_values(fake, None, 0, 1, C.byref(h)) == -1
    assert lib.dint_doc_filter_create_from_values(fake, fake, 0, 1, None) == -1 and h.value == 77


def test_from_float32_is_strictly_monotone():
    from dint_amd import device

    tiny = np.float32(1e-45)  # the smallest subnormal
    x = np.array([-np.inf, -3.4e38, -1.5, -1.0, -np.float32(1e-39), -tiny, -0.0, 0.0, tiny, np.float32(1e-39), np.float32(1.17549435e-38), 0.5, 1.0,
                  np.nextafter(np.float32(1.0), np.float32(2.0)), 3.4e38, np.inf], dtype=np.float32)
    rng = np.random.default_rng(1)
    more = np.unique(rng.integers(0, 1 << 32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32))
    more = more[~np.isnan(more) & (more != 0)]
    x = np.concatenate([x, more[~np.isin(more, x)]])
    order = np.lexsort((np.signbit(x) == 0, x))  # by value, -0.0 directly below +0.0
    x = x[order]
    keys = device.DocValues.float32_keys(x)
    assert keys.dtype == np.uint32 and (np.diff(keys.astype(np.int64)) > 0).all()
    z = device.DocValues.float32_keys(np.array([-0.0, 0.0], dtype=np.float32))
    assert z.tolist() == [0x7FFFFFFF, 0x80000000]
    assert device.DocValues.float32_keys(np.array([-np.inf, np.inf], dtype=np.float32)).tolist() == [0x007FFFFF, 0xFF800000]
    with pytest.raises(ValueError):
        device.DocValues.float32_keys(np.array([0.0, np.nan], dtype=np.float32))


# ---- the model ----------------------------------------------------------------------------------------------------------
def _same(x, y):
    return all(np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes() if isinstance(a, np.ndarray)
               else a == b for a, b in zip(x, y))


def test_the_special_cursors():
    sc = np.array([2.0, 2.0, 1.0, 1.0, 1.0, 0.5], dtype=np.float32)
    ids = np.array([3, 9, 1, 4, 8, 0], dtype=np.uint32)
    m = (sc, ids)
    values = np.array([M32, 7, 0, 5, 7, 0, 0, 0, 7], dtype=np.uint32)  # (document 9 is past the column: value 0)
    # descending: 0 (M32), 4 (7), 8 (7), 1 (7), 3 (5), 9 (0)
    assert DV.sorted_page(m, None, values, True, None, 4)[2].tolist() == [0, 1, 4, 8]
    assert DV.sorted_page(m, None, values, True, None, 6)[1].tolist() == [M32, 7, 7, 7, 5, 0]
    assert DV.sorted_page(m, None, values, True, None, 6)[3].tolist() == [0.5, 1.0, 1.0, 1.0, 2.0, 2.0]  # every hit keeps its score
    # ascending: 9 (0), 3 (5), 1, 4, 8 (7), 0 (M32): equal values by ascending docID in both orders
    assert DV.sorted_page(m, None, values, False, None, 6)[2].tolist() == [9, 3, 1, 4, 8, 0]
    # the all-ones keys: (0xFFFFFFFF, 0) descending and (0, 0) ascending are legitimate cursors that drop exactly document 0
    assert DV.key_of(M32, 0, True) == DV.key_of(0, 0, False) == 0xFFFFFFFFFFFFFFFF
    got = DV.sorted_page(m, None, values, True, (M32, 0), 6)
    assert got[0] == 5 and got[5] == 1 and got[2][:5].tolist() == [1, 4, 8, 3, 9]
    zeros = np.zeros(9, dtype=np.uint32)
    got = DV.sorted_page(m, None, zeros, False, (0, 0), 6)
    assert got[0] == 5 and got[5] == 1 and got[2][:5].tolist() == [1, 3, 4, 8, 9]
    # an unset cursor: from the start, whatever value it would have carried
    assert _same(DV.sorted_page(m, None, values, True, None, 3), DV.sorted_page_by_loop(m, None, values, True, None, 3))
    # a tie across the cursor: a match, a docID that is no match between two matched ones, docID 0 and 0xFFFFFFFF
    assert DV.sorted_page(m, None, values, True, (7, 4), 4)[2].tolist() == [8, 3, 9, M32] and DV.sorted_page(m, None, values, True, (7, 4), 4)[5] == 3
    assert DV.sorted_page(m, None, values, True, (7, 5), 4)[2][:2].tolist() == [8, 3] and DV.sorted_page(m, None, values, True, (7, 0), 4)[5] == 1
    assert DV.sorted_page(m, None, values, True, (7, M32), 4)[2][0] == 3 and DV.sorted_page(m, None, values, False, (7, M32), 4)[2][0] == 0
    # a value next to a match's: cuts in front of it or behind it
    assert DV.sorted_page(m, None, values, True, (8, 0), 4)[5] == 1 and DV.sorted_page(m, None, values, True, (6, M32), 4)[5] == 4
    for desc in (True, False):
        for cur in (None, (7, 4), (7, 5), (M32, 0), (0, 0), (0, M32), (M32, M32), (5, 3), (6, 0), (0, 9)):
            for k in (1, 3, 10):
                assert _same(DV.sorted_page(m, None, values, desc, cur, k), DV.sorted_page_by_loop(m, None, values, desc, cur, k)), (desc, cur, k)


def test_values_mask():
    v = np.array([0, 3, M32, 5, 3], dtype=np.uint32)
    assert DV.values_mask(v, 0, M32).all() and DV.values_mask(v, 3, 3).tolist() == [False, True, False, False, True]
    assert not DV.values_mask(v, 4, 2).any() and not DV.values_mask(v, 6, 1000).any() and DV.values_mask(v, M32, M32).tolist()[2]
    assert DV.values_mask(np.zeros(0, dtype=np.uint32), 0, M32).size == 0


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_per_document_loop_on_the_keys(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 4, x.size).astype(np.uint32) for x in lists]
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = np.ones(num_docs, dtype=np.float32) if seed % 2 else ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    bl = ranked.BuilderLists(docids, fr, bounds)
    kind, values, _ = DV.fuzz_values(r, num_docs)
    if seed == 3:
        values = values[:num_docs // 3]  # a column shorter than the index
    splits = ties = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], []):
            every = DV.DF.every_match(bl, q, nl, num_docs, conjunctive)
            for n_mask in (None, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                for desc in (True, False):
                    v, ids, sc = DV.in_order(every, mask, values, desc)
                    cursors = [None, (M32, 0), (0, 0), (0, M32), (M32, M32)] + ([DV.draw_cursor(r, v, ids, num_docs) for _ in range(8)] if ids.size else [])
                    for cur in cursors:
                        for k in (1, 10, 1000):
                            got = DV.sorted_page(every, mask, values, desc, cur, k)
                            assert _same(got, DV.sorted_page_by_loop(every, mask, values, desc, cur, k)), (q, desc, cur, k)
                            assert got[0] == min(k, got[4] - got[5])
                            hv = got[1][:got[0]].astype(np.int64)
                            assert (np.diff(hv) <= 0).all() if desc else (np.diff(hv) >= 0).all()
                        c = DV.conditions(every, mask, values, desc, cur, 3)
                        splits, ties = splits + c[2], ties + c[3]
                    # a walk by the last hit: the pages concatenate to the whole order, skipped counts the hits before
                    cur, seen = None, []
                    while True:
                        n, hv, d, s, m, skipped = DV.sorted_page(every, mask, values, desc, cur, 7)
                        assert skipped == len(seen) and m == ids.size
                        seen += d[:n].tolist()
                        if n < 7:
                            break
                        cur = DV.last_hit(n, hv, d)
                    assert seen == ids.tolist()
    assert splits > 30 and (ties > 5 or kind in ("wide", "docid", "reverse"))


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_draws_meet_their_conditions():
    """tests/test_gpu_doc_values_fuzz.py asserts four conditions on the device's own outputs (check_shares there). They are
    properties of the committed seeds and the draws: replayed here from the model, so that they are settled without a device,
    with the figures of that file."""
    import test_gpu_doc_values_fuzz as P

    totals = []
    for seed, kind, ds, fs in P.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = P.Z.F.make_dictionary(r, kind, **ds), P.Z.F.make_dictionary(r, kind, **fs)
        for i in range(P.CASES_PER_DICTIONARY):
            totals.append(P.model_shares(P.Y.draw_collapse_case(Dd, Df, 100 * seed + i)))
    assert len(totals) == 240
    P.check_shares(np.sum(totals, axis=0))
    assert [tuple(t) for t in np.sum(totals, axis=0).tolist()] == [P.FIGURES["or"], P.FIGURES["and"]]


# ---- the --values file parser -------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cstdio>
#include <iostream>
#include <string>
#include "%s"
int main(int argc, char** argv) {
    try {
        if (argc > 1) {
            uint32_t lo = 7, hi = 7;
            tool::parse_value_range(argv[1], lo, hi);
            std::printf("%%u %%u\n", lo, hi);
            return 0;
        }
        const tool::doc_values_column c = tool::parse_doc_values(std::cin);
        std::printf("%%llu %%zu", (unsigned long long)c.num_docs, c.values.size());
        for (uint32_t v : c.values) std::printf(" %%u", v);
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
    assert cxx, "g++ is needed to compile the values file parser"
    tmp = tmp_path_factory.mktemp("doc_values_file")
    src, exe = os.path.join(tmp, "parse.cpp"), os.path.join(tmp, "parse")
    with open(src, "w") as f:
        f.write(PROGRAM % PARSER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    return exe


def _parse(exe, text):
    """-> the column as a list, or None for a refused file"""
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    if out[0] == "error":
        return None
    v = [int(x) for x in out[2:]]
    assert len(v) == int(out[0]) == int(out[1])
    return v


def test_values_files(parser_exe):
    assert _parse(parser_exe, "") == [] and _parse(parser_exe, "\n  \n") == []
    assert _parse(parser_exe, "3 9\n") == [0, 0, 0, 9]  # unset documents: 0
    assert _parse(parser_exe, "  1:3   4294967295  \r\n\n5\t2\n") == [0, M32, M32, 0, 0, 2]
    assert _parse(parser_exe, "7:7 9\n9:3 1\n") == []  # empty and inverted intervals name no document
    assert _parse(parser_exe, "0:4 1\n2 5\n") == [1, 1, 5, 1] and _parse(parser_exe, "2 5\n0:4 1\n") == [1, 1, 1, 1]  # later lines win
    for bad in ("5\n", "5 1 2\n", "x 1\n", "5 -1\n", "5 4294967296\n", "4294967295 1\n", "1:x 2\n", "5 0x10\n"):
        assert _parse(parser_exe, bad) is None, bad
    rng = lambda a: subprocess.run([parser_exe, a], check=True, capture_output=True, text=True).stdout.split()  # noqa: E731
    assert rng("3:6") == ["3", "6"] and rng("9:2") == ["9", "2"] and rng("0:4294967295") == ["0", "4294967295"]
    for bad in ("3", "3:", ":3", "3:4294967296", "a:b", "1:2:3"):
        assert rng(bad)[0] == "error", bad
