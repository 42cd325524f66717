"""Ranked AND queries without a GPU: the C ABI's new entries and their argument checks, the host library's wand data
against the binary32 model (tests/ranked.py), the .sizes and wand data files, dint_create_wand_data, and the model itself
against its float64 form and the plain intersection."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ranked
from dint_amd import host
from queries import heavy_queries, intersect_freqs, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1
NEW = ("dint_wand_data_create", "dint_wand_data_destroy", "dint_ranked_and_queries")


def _wand_inputs(ix):
    num_docs = int(ix.docids.max()) + 1
    return host.sizes_from_postings(ix.docids, ix.freqs, num_docs), num_docs


def test_the_entries_are_exported_and_listed():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    for name in NEW:
        assert hasattr(lib, name)
        assert name in device.ABI_SYMBOLS
    assert device.WandData.MAX_K == 1024
    assert not set(device.OPTIONS) & {"query_ranked", "ranked"}


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    nl = np.ones(4, dtype=np.float32)
    wd = C.c_void_p()
    assert lib.dint_wand_data_create(0, nl.ctypes.data, 4, None) == DINT_ERR_ARG
    assert lib.dint_wand_data_create(0, None, 4, C.byref(wd)) == DINT_ERR_ARG
    lib.dint_wand_data_destroy(None)
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    ids = np.zeros(2048, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments are refused first)
    call = lib.dint_ranked_and_queries
    for qi, fd, w, k in ((None, fake, fake, 10), (fake, None, fake, 10), (fake, fake, None, 10), (None, None, None, 10),
                         (fake, fake, fake, 0), (fake, fake, fake, 1025), (fake, fake, fake, 1 << 31)):
        assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data, scores.ctypes.data,
                    ids.ctypes.data, None) == DINT_ERR_ARG
    assert call(None, None, None, 10, None, None, 0, None, None, None, None) == DINT_ERR_ARG


@pytest.mark.parametrize("corpus_name", ["small_corpus", "sparse_corpus"])
def test_host_wand_data_is_bit_equal_to_the_model(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    sizes, num_docs = _wand_inputs(ix)
    nl, mtw = host.wand_data(sizes, ix.docids, ix.freqs, ix.lens)
    want_nl = ranked.norm_lens(sizes)
    assert nl.dtype == np.float32 and nl.size == num_docs
    assert np.array_equal(nl.view(np.uint32), want_nl.view(np.uint32))
    want_mtw = ranked.max_term_weights(ix.docids, ix.freqs, ix.bounds, want_nl)
    assert np.array_equal(mtw.view(np.uint32), want_mtw.view(np.uint32))
    assert (mtw[ix.lens > 0] > 0).all() and (mtw < 1).all()
    # docIDs beyond the sizes are refused
    with pytest.raises(host.HostError):
        host.wand_data(sizes[: num_docs - 1], ix.docids, ix.freqs, ix.lens)


def test_sizes_and_wand_files_round_trip(tmp_path):
    sizes = np.array([3, 0, 7, 1 << 20, 5], dtype=np.uint32)
    host.write_sizes(str(tmp_path / "c.sizes"), sizes)
    assert np.array_equal(host.read_sizes(str(tmp_path / "c.sizes")), sizes)
    assert os.path.getsize(tmp_path / "c.sizes") == 4 * (1 + sizes.size)
    nl = np.array([0.5, 1.25, 2.0], dtype=np.float32)
    mtw = np.array([0.1, 0.7], dtype=np.float32)
    host.write_wand_data(str(tmp_path / "w"), nl, mtw)
    raw = (tmp_path / "w").read_bytes()
    assert len(raw) == 24 + 4 * 5 and raw[:4] == b"DWND"
    got_nl, got_mtw = host.read_wand_data(str(tmp_path / "w"))
    assert np.array_equal(got_nl, nl) and np.array_equal(got_mtw, mtw)
    (tmp_path / "bad").write_bytes(raw[:-1])
    with pytest.raises(host.HostError):
        host.read_wand_data(str(tmp_path / "bad"))
    with pytest.raises(host.HostError):
        host.read_sizes(str(tmp_path / "missing.sizes"))


def test_create_wand_data_tool(tmp_path, small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    sizes, num_docs = _wand_inputs(ix)
    b = ix.bounds
    base = str(tmp_path / "c")
    host.write_collection(base, [ix.docids[int(b[i]):int(b[i + 1])] for i in range(len(ix.lens))],
                          [ix.freqs[int(b[i]):int(b[i + 1])] for i in range(len(ix.lens))], num_docs=num_docs)
    host.write_sizes(base + ".sizes", sizes)
    tool = os.path.join(ROOT, "dint_amd", "bin", "dint_create_wand_data")
    r = subprocess.run([tool, base, str(tmp_path / "c.wand")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got_nl, got_mtw = host.read_wand_data(str(tmp_path / "c.wand"))
    want_nl, want_mtw = host.wand_data(sizes, ix.docids, ix.freqs, ix.lens)
    assert np.array_equal(got_nl.view(np.uint32), want_nl.view(np.uint32))
    assert np.array_equal(got_mtw.view(np.uint32), want_mtw.view(np.uint32))
    r = subprocess.run([tool, base], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "Usage" in r.stderr


def test_model_against_float64_and_the_intersection(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    sizes, num_docs = _wand_inputs(ix)
    nl = ranked.norm_lens(sizes)
    lists = ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds)
    qs = reference_queries(len(ix.lens))[:150] + heavy_queries(ix.lens, 20)
    checked = 0
    for q in qs:
        n_all = intersect_freqs(ix.docids, ix.freqs, ix.bounds, q)[0]
        k = max(1, n_all)
        count, scores, ids = ranked.ranked_and(lists, q, nl, num_docs, k)
        assert count == (n_all if len(q) else 0)
        if count == 0:
            continue
        f64 = ranked.ranked_and_f64(lists, q, nl, num_docs)
        assert set(ids[:count].tolist()) == set(f64)
        for s, d in zip(scores[:count].tolist(), ids[:count].tolist()):
            assert s > 0 and abs(s - f64[d]) <= 1e-6 * f64[d] * max(4, 2 * len(q))
        assert (np.diff(scores[:count]) <= 0).all()
        ties = np.diff(scores[:count]) == 0
        assert (np.diff(ids[:count].astype(np.int64))[ties] > 0).all()
        checked += count
    assert checked > 10_000


def test_idf_clamp_and_query_weight():
    # df above num_docs / 2: the idf is negative and clamped to 1e-6
    assert ranked.query_term_weight(1, 900, 1000) == np.float32(1e-6) * np.float32(2.2)
    assert ranked.query_term_weight(2, 10, 1000) > ranked.query_term_weight(1, 10, 1000)
    assert ranked.query_term_weight(1, 10, 1000) == np.float32(1) * ranked.logf(np.float32(990.5) / np.float32(10.5)) * np.float32(2.2)
