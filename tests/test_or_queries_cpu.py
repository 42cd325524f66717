"""OR queries without a GPU: the C ABI's new entries and option, and the expected values the GPU tests compare with —
plain set union of the index builder's input against the union of the lists the CPU oracle decodes from the index."""
import ctypes as C
import os

import numpy as np
import pytest

from dint_amd import host
from or_union import oracle_lists, union, union_freqs
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1


def test_the_entries_are_exported_and_listed():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    for name in ("dint_or_queries", "dint_or_queries_freqs"):
        assert hasattr(lib, name)
        assert name in device.ABI_SYMBOLS


def test_a_null_query_index_is_a_bad_argument():
    from dint_amd import device

    lib = device._lib
    counts = np.zeros(1, dtype=np.uint64)
    sums = np.zeros(1, dtype=np.uint64)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    nblocks = C.c_uint64(7)
    assert lib.dint_or_queries(None, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data, None) == DINT_ERR_ARG
    assert lib.dint_or_queries_freqs(None, None, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data,
                                     sums.ctypes.data, C.byref(nblocks), None) == DINT_ERR_ARG
    assert lib.dint_or_queries(None, None, None, 0, None, None) == DINT_ERR_ARG


def test_the_pass_bound_is_an_option():
    from dint_amd import device

    lib = device._lib
    n = device.LIMITS["query_or_pass_pages"]
    assert lib.dint_option_name(n) == b"query_or_pass_pages"
    assert "query_or_pass_pages" not in device.OPTIONS  # (a bound, not one of the code-path switches)
    device.reset_options()
    assert device.get_option("query_or_pass_pages") == 1 << 20  # 1 GiB of docIDs a pass
    for bad in (0, -1, 1 << 32):
        assert lib.dint_set_option(n, C.c_longlong(bad)) == DINT_ERR_ARG
    with pytest.raises(device.DintError):
        device.set_option("query_or_pass_pages", 0)
    with device.options(query_or_pass_pages=7):
        assert device.get_option("query_or_pass_pages") == 7
    assert device.get_option("query_or_pass_pages") == 1 << 20
    device.set_option("query_or_pass_pages", (1 << 32) - 1)
    device.reset_options()
    assert device.get_option("query_or_pass_pages") == 1 << 20


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
def test_set_union_is_the_union_of_the_oracle_decoded_lists(small_corpus, kind):
    ix = get_index(small_corpus, kind)
    ol = oracle_lists(ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 20, seed=4)
    total = 0
    for q in qs:
        want = union(ix.docids, ix.bounds, q)
        assert ol.union(q) == want
        total += want
    assert total > 100_000
    q = qs[-1]
    _, fsum = union_freqs(ix.docids, ix.freqs, ix.bounds, q)
    assert fsum == sum(int(ol.postings(int(t))[1].astype(np.uint64).sum()) for t in np.unique(q))
