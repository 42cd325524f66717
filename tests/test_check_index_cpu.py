"""dint_check_index without a GPU: the header declares the call, its two structs and the four DINT_CHECK_* values, the binding
registers them, the ABI version is still 6, the refusals that touch no device are DINT_ERR_ARG, and the model of
tests/check_index.py agrees with expectations written by hand on a three-list toy; the tool's refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np

import check_index as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1


def test_the_header_declares_the_call_the_structs_and_the_kinds():
    text = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert "#define DINT_CHECK_LENGTH 1 /* verify_collection.hpp:18-24 */" in text  # (the kinds cite the reference's lines)
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "int dint_check_index(dint_query_index* qi, const dint_dict* freqs_dict, const dint_collection_view* view," in header
    for name, value in (("OK", 0), ("LENGTH", 1), ("DOCID", 2), ("FREQ", 3)):
        assert re.search(rf"#define DINT_CHECK_{name}\s+{value}\b", header), name
    view = header.split("typedef struct dint_collection_view {")[1].split("} dint_collection_view;")[0]
    assert re.findall(r"(\w+);", view) == ["docs", "freqs", "docs_at", "freqs_at", "list_len", "n_lists"]
    mismatch = header.split("typedef struct dint_index_mismatch {")[1].split("} dint_index_mismatch;")[0]
    assert re.findall(r"(uint\d+_t) (\w+);", mismatch) == [("uint32_t", "kind"), ("uint32_t", "list"), ("uint64_t", "position"),
                                                           ("uint64_t", "expected"), ("uint64_t", "got")]
    # a section of its own behind dint_index_max_weights
    assert header.index("int dint_index_max_weights(") < header.index("int dint_check_index(")
    assert "#define DINT_ABI_VERSION 6" in header


def test_the_binding_registers_the_call_and_the_structs():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    assert hasattr(lib, "dint_check_index")
    assert "dint_check_index" in device.ABI_SYMBOLS
    assert hasattr(device.QueryIndex, "check")
    assert device.abi_version() == 6
    assert [n for n, _ in device.CollectionView._fields_] == ["docs", "freqs", "docs_at", "freqs_at", "list_len", "n_lists"]
    assert C.sizeof(device.CollectionView) == 48
    assert [n for n, _ in device.IndexMismatch._fields_] == ["kind", "list", "position", "expected", "got"]
    assert C.sizeof(device.IndexMismatch) == 32 and device.IndexMismatch.position.offset == 8
    assert (device.CHECK_OK, device.CHECK_LENGTH, device.CHECK_DOCID, device.CHECK_FREQ) == (M.OK, M.LENGTH, M.DOCID, M.FREQ) == (0, 1, 2, 3)
    assert device.Mismatch._fields == M.Mismatch._fields == ("kind", "list", "position", "expected", "got")
    assert device._lib.dint_check_index.argtypes[2:5] == [C.POINTER(device.CollectionView), C.POINTER(C.c_uint64),
                                                          C.POINTER(device.IndexMismatch)]
    # no new option
    assert list(device.LIMITS) == ["query_or_pass_pages"] and not [o for o in device.OPTIONS if "check" in o]


def test_null_arguments_are_refused_without_a_device():
    from dint_amd import device

    call = device._lib.dint_check_index
    view, n, first = device.CollectionView(), C.c_uint64(7), device.IndexMismatch()
    fake = C.c_void_p(8)  # never read: the null checks come first
    assert call(None, None, C.byref(view), C.byref(n), C.byref(first), None) == DINT_ERR_ARG   # no query index
    assert call(fake, None, None, C.byref(n), C.byref(first), None) == DINT_ERR_ARG            # no view
    assert call(fake, None, C.byref(view), None, C.byref(first), None) == DINT_ERR_ARG         # nowhere to count
    assert call(None, None, None, None, None, None) == DINT_ERR_ARG
    assert n.value == 7 and first.kind == 0


def toy():
    lists = [np.array([2, 5, 9], np.uint32), np.array([0, 1, 4, 7], np.uint32), np.array([3, 8], np.uint32)]
    freqs = [np.array([1, 2, 1], np.uint32), np.array([3, 1, 1, 2], np.uint32), np.array([5, 6], np.uint32)]
    return lists, freqs


def test_the_model_on_a_three_list_toy():
    lists, freqs = toy()
    assert M.check(lists, freqs, M.view_of(lists, freqs)) == (0, None)
    assert M.check(lists, None, M.view_of(lists)) == (0, None)

    # a docID and a freq wrong at the same position: DOCID reported, counted once
    v = M.view_of(lists, freqs)
    v.docs[int(v.docs_at[1]) + 2] = 6
    v.freqs[int(v.freqs_at[1]) + 2] = 9
    assert M.check(lists, freqs, v) == (1, M.Mismatch(M.DOCID, 1, 2, 6, 4))
    # ... and docIDs only sees the same
    assert M.check(lists, freqs, v, with_freqs=False) == (1, M.Mismatch(M.DOCID, 1, 2, 6, 4))

    # a freq alone
    v = M.view_of(lists, freqs)
    v.freqs[int(v.freqs_at[2]) + 1] = 7
    assert M.check(lists, freqs, v) == (1, M.Mismatch(M.FREQ, 2, 1, 7, 6))
    assert M.check(lists, freqs, v, with_freqs=False) == (0, None)

    # a wrong length: one mismatch, none of the list's postings compared (the view's list 1 is a posting longer and its
    # third docID is wrong as well); an earlier list beats a later one
    longer = [lists[0], np.array([0, 1, 5, 7, 11], np.uint32), lists[2]]
    longer_f = [freqs[0], np.array([3, 1, 1, 2, 1], np.uint32), freqs[2]]
    v = M.view_of(longer, longer_f)
    assert M.check(lists, freqs, v) == (1, M.Mismatch(M.LENGTH, 1, 0, 5, 4))
    v.docs[int(v.docs_at[2])] = 1      # list 2, position 0: later than the length
    assert M.check(lists, freqs, v) == (2, M.Mismatch(M.LENGTH, 1, 0, 5, 4))
    v.freqs[int(v.freqs_at[0]) + 2] = 4  # list 0, position 2: earlier
    assert M.check(lists, freqs, v) == (3, M.Mismatch(M.FREQ, 0, 2, 4, 1))
    v.docs[int(v.docs_at[0]) + 1] = 0xFFFFFFFF  # list 0, position 1: earlier still
    assert M.check(lists, freqs, v) == (4, M.Mismatch(M.DOCID, 0, 1, 0xFFFFFFFF, 5))


def test_the_tool_refuses_before_it_touches_a_device(tmp_path):
    """An index type other than the file's, a collection with another number of lists, a truncated collection file: exit
    status 1 and a message, all before the device is asked for."""
    import subprocess

    from dint_amd import host

    coll = host.synth_collection(20_000, universe=15_000, seed=53)
    docids, freqs, b = host.gaps_to_docids(coll), host.synth_freqs(coll.num_postings, 13), coll.list_bounds()
    n = len(coll.lens)
    lists = [docids[int(b[i]):int(b[i + 1])] for i in range(n)]
    fl = [freqs[int(b[i]):int(b[i + 1])] for i in range(n)]
    num_docs = int(docids.max()) + 1
    host.write_collection(str(tmp_path / "c"), lists, fl, num_docs=num_docs)
    host.write_collection(str(tmp_path / "fewer"), lists[:-1], fl[:-1], num_docs=num_docs)
    (tmp_path / "cut.docs").write_bytes((tmp_path / "c.docs").read_bytes()[:-40])
    (tmp_path / "cut.freqs").write_bytes((tmp_path / "c.freqs").read_bytes())
    bin_ = lambda name: os.path.join(ROOT, "dint_amd", "bin", name)
    run = lambda *a: subprocess.run(list(a), cwd=tmp_path, capture_output=True, text=True, timeout=300)
    r = run(bin_("dint_create_freq_index"), "single_packed_dint", "c", "c.index", "--threads", "2", "--check")
    assert r.returncode == 0 and "dint_check_index" in r.stderr  # (--check names the tool that checks)
    for args, message in ((("multi_packed_dint", "c.index", "c"), "another index type"),
                          (("single_packed_dint", "c.index", "fewer"), f"{n - 1} sequences, the index {n}"),
                          (("single_packed_dint", "c.index", "cut"), "cut.docs is truncated"),
                          (("no_such_dint", "c.index", "c"), "Unknown type")):
        r = run(bin_("dint_check_index"), *args)
        assert r.returncode == 1 and message in r.stderr and r.stdout == "", (args, r.stderr)
    assert run(bin_("dint_check_index"), "single_packed_dint", "c.index").returncode == 1  # usage
