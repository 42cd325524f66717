"""Ranked AND queries on the GPU through the C ABI (dint_ranked_and_queries): counts, BM25 scores and docIDs bit-equal to the
binary32 model of ranked_and_query (tests/ranked.py; include/ds2i/queries.hpp:309-385) over the index builder's input and
over the lists the CPU oracle decodes from the index."""
import ctypes as C
import threading

import numpy as np
import pytest

import ranked
from dint_amd import host
from or_union import oracle_lists
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available()
    from dint_amd import device as dev

    return dev


@pytest.fixture(autouse=True)
def _options_back_to_default(device):
    yield
    device.reset_options()


class Ranked:
    """An index on the device with its freqs dictionary and wand data (sizes: the sums of the documents' freqs)."""

    def __init__(self, device, ix, kind, num_docs=None):
        self.ix = ix
        self.num_docs = num_docs or int(ix.docids.max()) + 1
        self.sizes = host.sizes_from_postings(ix.docids, ix.freqs, self.num_docs)
        self.norm_lens, _ = host.wand_data(self.sizes, ix.docids, ix.freqs, ix.lens)
        self.qi = device.QueryIndex(device.Dictionary(kind, ix.docs_dict), ix.bytes, ix.offsets)
        self.fd = device.Dictionary(kind, ix.freqs_dict)
        self.wand = device.WandData(self.norm_lens)
        self.lists = ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds)

    def run(self, qs, k):
        return self.qi.ranked_and_queries(self.fd, self.wand, qs, k=k)

    def want(self, qs, k, lists=None):
        lists = lists or self.lists
        out = [ranked.ranked_and(lists, q, self.norm_lens, self.num_docs, k) for q in qs]
        return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]) if out else np.zeros((0, k), np.float32),
                np.stack([o[2] for o in out]) if out else np.zeros((0, k), np.uint32))

    def close(self):
        self.qi.close()
        self.wand.close()


def _assert_equal(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))  # bit-equal scores
    assert np.array_equal(got[2], want[2])


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_is_bit_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Ranked(device, ix, kind)
    qs = reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 120)
    ol = oracle_lists(ix, kind)
    sample = qs[::11]
    for k in (10, 1, 1000):
        got = r.run(qs, k)
        want = r.want(qs, k)
        _assert_equal(got, want)
        if k == 10:
            assert int(want[0].sum()) > 500
            idx = list(range(0, len(qs), 11))
            _assert_equal(tuple(a[idx] for a in got), r.want(sample, k, lists=ol))
    r.close()


def test_edges(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    longest = int(np.argmax(ix.lens))
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    qs = [[], [mid], [longest], [mid, mid], [mid, longest], [longest, mid, longest]]
    got = r.run(qs, 10)
    _assert_equal(got, r.want(qs, 10))
    assert got[0][0] == 0 and (got[1][0] == 0).all() and (got[2][0] == 0xFFFFFFFF).all()
    assert got[0][1] == 10 and got[0][2] == 10
    # [t, t] weighs twice [t]: every score from q_weight(qf = 2)
    assert (got[1][3] > got[1][1]).all()
    # k larger than the intersection: count = matches, the rest empty
    big = r.run([[mid]], 1000)
    n = int(big[0][0])
    assert n == ix.lens[mid] and (big[2][0][n:] == 0xFFFFFFFF).all() and (big[1][0][n:] == 0).all()
    _assert_equal(big, r.want([[mid]], 1000))
    with pytest.raises(device.DintError):
        r.run([[len(ix.lens)]], 10)
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            r.run([[mid]], bad_k)
    r.close()


def _hand_made(device, kind):
    """Lists with an empty intersection, a list longer than num_docs / 2 and equal scores."""
    a = np.arange(0, 3000, dtype=np.uint32)
    b = np.arange(5000, 9000, dtype=np.uint32)            # disjoint from a
    c = np.arange(0, 9000, 2, dtype=np.uint32)            # 4500 of 9000 documents
    d = np.arange(0, 9000, dtype=np.uint32)               # df = num_docs: clamped idf
    e = np.array([10, 20, 30, 40], dtype=np.uint32)
    lists = [a, b, c, d, e]
    lens = np.array([x.size for x in lists], dtype=np.uint32)
    docids = np.concatenate(lists)
    freqs = np.ones(docids.size, dtype=np.uint32)          # equal freqs, equal sizes below: equal scores
    freqs[lens[0]:lens[0] + 7] = 3
    gaps = np.concatenate([host.docids_to_gaps(x) for x in lists])
    coll = host.Collection(gaps, lens)
    dd = host.build_dictionary(kind, coll)
    fd = host.build_dictionary(kind, host.Collection(freqs - 1, lens))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, lens)

    class Ix:
        pass

    ix = Ix()
    ix.docids, ix.freqs, ix.lens, ix.bounds = docids, freqs, lens, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    ix.docs_dict, ix.freqs_dict, ix.bytes, ix.offsets = dd, fd, idx, offs
    return ix


def test_empty_intersection_clamped_idf_and_ties(device):
    kind = host.MULTI_PACKED
    ix = _hand_made(device, kind)
    r = Ranked(device, ix, kind, num_docs=9000)
    # sizes: make every document the same length so equal freqs give equal scores
    r.norm_lens = np.ones(9000, dtype=np.float32)
    r.wand = device.WandData(r.norm_lens)
    qs = [[0, 1], [3], [3, 4], [2, 4], [0, 2], [4]]
    got = r.run(qs, 10)
    _assert_equal(got, r.want(qs, 10))
    assert got[0][0] == 0
    w3 = ranked.query_term_weight(1, 9000, 9000)
    assert w3 == np.float32(1e-6) * np.float32(2.2)  # the clamp
    assert got[0][1] == 10 and np.array_equal(got[2][1], np.arange(10))  # all tied: ascending docIDs
    assert np.array_equal(got[2][5], [10, 20, 30, 40, *[0xFFFFFFFF] * 6])
    assert len(set(got[1][5][:4].tolist())) == 1  # tie among the four
    r.close()


def test_batch_equals_one_at_a_time(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:60] + heavy_queries(ix.lens, 12)
    batch = r.run(qs, 10)
    for i, q in enumerate(qs):
        one = r.run([q], 10)
        _assert_equal(one, tuple(a[i:i + 1] for a in batch))
    r.close()


@pytest.mark.parametrize("opts", [dict(query_fused_pages=0), dict(query_tail_pages=0, query_fused_pages=0),
                                  dict(query_lean_pages=0), dict(query_lean_pages=1 << 30, query_tail_pages=1 << 20)])
def test_forms_through_the_options(device, dense_corpus, opts):
    kind = host.RECTANGULAR
    ix = get_index(dense_corpus, kind)
    r = Ranked(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 10)
    want = r.want(qs, 10)
    with device.options(**opts):
        _assert_equal(r.run(qs, 10), want)
        _assert_equal(r.run(qs[-1:], 10), tuple(a[-1:] for a in want))
    r.close()


def test_a_short_wand_handle_is_refused_before_any_launch(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    top = int(ix.docids.max())
    short = device.WandData(r.norm_lens[:top])  # num_docs == the largest docID
    with pytest.raises(device.DintError):
        r.qi.ranked_and_queries(r.fd, short, [[0]], k=10)
    lib = device._lib
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    assert lib.dint_ranked_and_queries(r.qi._h, r.fd._h, short._h, 10, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data,
                                       scores.ctypes.data, None, None) == DINT_ERR_ARG
    # docids may be null
    ok = device.WandData(r.norm_lens)
    assert lib.dint_ranked_and_queries(r.qi._h, r.fd._h, ok._h, 10, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data,
                                       scores.ctypes.data, None, None) == 0
    want = r.want([[0]], 10)
    assert counts[0] == want[0][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))
    # a freqs dictionary of another kind
    other = device.Dictionary(host.MULTI_PACKED, get_index(small_corpus, host.MULTI_PACKED).freqs_dict)
    with pytest.raises(device.DintError):
        r.qi.ranked_and_queries(other, ok, [[0]], k=10)
    short.close()
    ok.close()
    r.close()


def test_ranked_and_or_interleaved_and_two_threads(device, small_corpus):
    from queries import intersect
    from or_union import union

    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    want = r.want(qs, 10)
    want_and = np.array([intersect(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    want_or = np.array([union(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    for _ in range(2):
        _assert_equal(r.run(qs, 10), want)
        assert np.array_equal(r.qi.and_queries(qs), want_and)
        assert np.array_equal(r.qi.or_queries(qs), want_or)
        assert np.array_equal(r.qi.and_queries_with_freqs(r.fd, qs)[0], want_and)
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            for _ in range(3):
                if which == 0:
                    _assert_equal(r.run(qs, 10), want)
                else:
                    assert np.array_equal(r.qi.and_queries(qs), want_and)
                    _assert_equal(r.run(qs[::-1], 10), tuple(a[::-1] for a in want))
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    r.close()
