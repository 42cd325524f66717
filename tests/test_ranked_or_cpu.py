"""Ranked OR queries without a GPU: the C ABI's new entry and its argument checks, and the binary32 model
(tests/ranked_or.py) against its float64 form, the plain set union and a direct transcription of ranked_or_query's cursor
loop and topk_queue (include/ds2i/queries.hpp:150-188, :387-457)."""
import ctypes as C
import heapq
import os

import numpy as np
import pytest

import ranked
import ranked_or
from dint_amd import host
from or_union import union
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1
F = np.float32


def _wand_inputs(ix):
    num_docs = int(ix.docids.max()) + 1
    return host.sizes_from_postings(ix.docids, ix.freqs, num_docs), num_docs


def test_the_entry_is_exported_and_listed():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    assert hasattr(lib, "dint_ranked_or_queries")
    assert "dint_ranked_or_queries" in device.ABI_SYMBOLS
    assert hasattr(device.QueryIndex, "ranked_or_queries")
    assert device.abi_version() == 6
    assert not set(device.OPTIONS) & {"query_ranked_or", "ranked_or"}


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    ids = np.zeros(2048, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and the bad k are refused first)
    call = lib.dint_ranked_or_queries
    for qi, fd, w, k in ((None, fake, fake, 10), (fake, None, fake, 10), (fake, fake, None, 10), (None, None, None, 10),
                         (fake, fake, fake, 0), (fake, fake, fake, 1025), (fake, fake, fake, 1 << 31)):
        assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data, scores.ctypes.data,
                    ids.ctypes.data, None) == DINT_ERR_ARG
    assert call(None, None, None, 10, None, None, 0, None, None, None, None) == DINT_ERR_ARG


def _cursor_loop(lists, terms, nl, num_docs: int, k: int):
    """ranked_or_query transcribed: the cursors in query_freqs order, the sum from 0 at every current docID, topk_queue's
    min-heap of k floats (insert: push while short, else replace the smallest when strictly greater) -> the sorted top-k."""
    if len(terms) == 0:
        return []
    t, qf = ranked.query_freqs(terms)
    enums = []
    for x, m in zip(t.tolist(), qf.tolist()):
        d, f = lists.postings(int(x))
        enums.append([d, f, 0, ranked.query_term_weight(int(m), int(d.size), num_docs)])
    end = 1 << 40
    docid = lambda e: int(e[0][e[2]]) if e[2] < e[0].size else end
    cur = min(docid(e) for e in enums)
    heap = []
    while cur < end:
        score = F(0)
        norm_len = F(nl[cur])
        nxt = end
        for e in enums:
            if docid(e) == cur:
                score = score + e[3] * ranked.doc_term_weight(F(e[1][e[2]]), norm_len)
                e[2] += 1
            nxt = min(nxt, docid(e))
        if len(heap) < k:
            heapq.heappush(heap, float(score))
        elif float(score) > heap[0]:
            heapq.heapreplace(heap, float(score))
        cur = nxt
    return sorted(heap, reverse=True)


def test_model_against_float64_and_the_union(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    sizes, num_docs = _wand_inputs(ix)
    nl = ranked.norm_lens(sizes)
    lists = ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 10)
    checked = 0
    for q in qs:
        n_all = union(ix.docids, ix.bounds, q)
        for k in (10, max(1, n_all)):
            count, scores, ids = ranked_or.ranked_or(lists, q, nl, num_docs, k)
            assert count == (min(k, n_all) if len(q) else 0)
            assert (ids[count:] == 0xFFFFFFFF).all() and (scores[count:] == 0).all()
            if count == 0:
                continue
            f64 = ranked_or.ranked_or_f64(lists, q, nl, num_docs)
            if k == n_all:
                assert set(ids[:count].tolist()) == set(f64)
                checked += count
            for s, d in zip(scores[:count].tolist(), ids[:count].tolist()):
                assert s > 0 and abs(s - f64[d]) <= 1e-6 * f64[d] * max(4, 2 * len(q))
            assert (np.diff(scores[:count]) <= 0).all()
            ties = np.diff(scores[:count]) == 0
            assert (np.diff(ids[:count].astype(np.int64))[ties] > 0).all()
    assert checked > 10_000


@pytest.mark.parametrize("seed", [3, 17])
def test_model_equals_the_cursor_loop_bit_for_bit(seed):
    coll = host.synth_collection(30_000, universe=4_000, seed=seed)
    docids = host.gaps_to_docids(coll)
    freqs = host.synth_freqs(coll.num_postings, seed)
    bounds = coll.list_bounds()
    num_docs = int(docids.max()) + 1
    nl = ranked.norm_lens(host.sizes_from_postings(docids, freqs, num_docs))
    lists = ranked.BuilderLists(docids, freqs, bounds)
    rng = np.random.default_rng(seed)
    n_lists = len(coll.lens)
    qs = [[], [0], [3, 3], [1, 2, 1]] + [rng.integers(0, n_lists, size=int(rng.integers(1, 6))).tolist() for _ in range(40)]
    compared = 0
    for q in qs:
        for k in (1, 10, 200):
            count, scores, _ = ranked_or.ranked_or(lists, q, nl, num_docs, k)
            want = _cursor_loop(lists, q, nl, num_docs, k)
            assert count == len(want)
            assert np.array_equal(scores[:count].view(np.uint32), np.array(want, dtype=np.float32).view(np.uint32))
            compared += count
    assert compared > 1000


def test_the_sum_runs_in_ascending_term_id():
    """Three terms whose weights, added in two orders, round apart: the model follows ascending term id, whatever the
    lists' lengths are."""
    lists = ranked.BuilderLists(np.array([0, 0, 1, 2, 0, 3, 4, 5, 6, 7, 8], dtype=np.uint32),
                                np.array([1, 7, 1, 1, 3, 1, 1, 1, 1, 1, 1], dtype=np.uint32), np.array([0, 1, 4, 11], dtype=np.uint64))
    nl = np.linspace(0.3, 2.1, 9).astype(np.float32)
    count, scores, ids = ranked_or.ranked_or(lists, [2, 0, 1], nl, 9, 9)
    assert count == 9 and ids[0] == 0
    w = [ranked.query_term_weight(1, n, 9) * ranked.doc_term_weight(F(f), nl[0]) for n, f in ((1, 1), (3, 7), (7, 3))]
    assert scores[0] == (F(0) + w[0] + w[1]) + w[2]
