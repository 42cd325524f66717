"""Ranked OR queries on the GPU through the C ABI (dint_ranked_or_queries): counts, BM25 scores and docIDs bit-equal to the
binary32 model of ranked_or_query (tests/ranked_or.py; include/ds2i/queries.hpp:387-457) over the index builder's input
and over the lists the CPU oracle decodes from the index."""
import threading

import numpy as np
import pytest

import ranked
import ranked_or
from dint_amd import host
from or_union import oracle_lists, union
from queries import ReadmeIndex, heavy_queries, intersect, reference_queries
from test_gpu_ranked_queries import Ranked, _assert_equal, _hand_made
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


class RankedOr(Ranked):
    def run(self, qs, k):
        return self.qi.ranked_or_queries(self.fd, self.wand, qs, k=k)

    def run_and(self, qs, k):
        return self.qi.ranked_and_queries(self.fd, self.wand, qs, k=k)

    def want(self, qs, k, lists=None):
        lists = lists or self.lists
        out = [ranked_or.ranked_or(lists, q, self.norm_lens, self.num_docs, k) for q in qs]
        return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]) if out else np.zeros((0, k), np.float32),
                np.stack([o[2] for o in out]) if out else np.zeros((0, k), np.uint32))

    def want_and(self, qs, k):
        out = [ranked.ranked_and(self.lists, q, self.norm_lens, self.num_docs, k) for q in qs]
        return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_is_bit_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = RankedOr(device, ix, kind)
    qs = reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 60)
    ol = oracle_lists(ix, kind)
    idx = list(range(0, len(qs), 11))
    sample = [qs[i] for i in idx]
    for k in (10, 1, 1000):
        got = r.run(qs, k)
        want = r.want(qs, k)
        _assert_equal(got, want)
        if k == 10:
            assert int(want[0].sum()) > 500
            assert np.array_equal(got[0], np.array([min(10, union(ix.docids, ix.bounds, q)) if len(q) else 0 for q in qs], dtype=np.uint64))
            _assert_equal(tuple(a[idx] for a in got), r.want(sample, k, lists=ol))
    r.close()


def test_edges(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = RankedOr(device, ix, kind)
    longest = int(np.argmax(ix.lens))
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    small = int(np.flatnonzero((ix.lens >= 1) & (ix.lens < 5))[0])
    qs = [[], [mid], [longest], [mid, mid], [mid, longest], [longest, mid, longest], [small], [small, small, mid]]
    got = r.run(qs, 10)
    _assert_equal(got, r.want(qs, 10))
    assert got[0][0] == 0 and (got[1][0] == 0).all() and (got[2][0] == 0xFFFFFFFF).all()
    assert got[0][1] == 10 and got[0][2] == 10
    assert got[0][6] == ix.lens[small] and (got[2][6][ix.lens[small]:] == 0xFFFFFFFF).all()
    # [t, t] weighs twice [t]: every score from q_weight(qf = 2)
    assert (got[1][3] > got[1][1]).all()
    # k larger than the union: count = |union|, the rest empty
    big = r.run([[mid], [small, mid]], 1000)
    n = int(big[0][0])
    assert n == ix.lens[mid] and (big[2][0][n:] == 0xFFFFFFFF).all() and (big[1][0][n:] == 0).all()
    assert int(big[0][1]) == union(ix.docids, ix.bounds, [small, mid])
    _assert_equal(big, r.want([[mid], [small, mid]], 1000))
    with pytest.raises(device.DintError):
        r.run([[len(ix.lens)]], 10)
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            r.run([[mid]], bad_k)
    r.close()


def test_disjoint_subset_clamped_idf_and_ties(device):
    """Lists a (0..2999) and b (5000..8999) are disjoint, c (the evens) and e (four docs) are subsets of d (every doc, the
    idf clamped); every document has the same length and most freqs are 1, so scores tie across terms."""
    kind = host.MULTI_PACKED
    ix = _hand_made(device, kind)
    r = RankedOr(device, ix, kind, num_docs=9000)
    r.norm_lens = np.ones(9000, dtype=np.float32)
    r.wand = device.WandData(r.norm_lens)
    qs = [[0, 1], [1, 0], [3], [3, 4], [4, 3], [2, 4], [0, 2], [4], [2, 3, 4], [0, 1, 4]]
    for k in (10, 1, 1000):
        got = r.run(qs, k)
        _assert_equal(got, r.want(qs, k))
    got = r.run(qs, 10)
    assert got[0][0] == 10 and got[0][2] == 10 and got[0][7] == 4
    # [0, 1]: a's documents tie (the rarer list, freq 1), by ascending docID; the term order of the query does not matter
    assert np.array_equal(got[2][0], np.arange(10)) and len(set(got[1][0].tolist())) == 1
    assert np.array_equal(got[2][1], got[2][0]) and np.array_equal(got[1][1].view(np.uint32), got[1][0].view(np.uint32))
    # [2, 4]: e's four documents (all even: in c too) score both terms, tied, above c's other documents (tied, clamped idf)
    assert np.array_equal(got[2][5][:4], [10, 20, 30, 40]) and len(set(got[1][5][:4].tolist())) == 1
    assert np.array_equal(got[2][5][4:], [0, 2, 4, 6, 8, 12])
    full = r.run([[0, 1], [2, 4]], 1000)
    assert full[0][0] == 1000 and full[0][1] == 1000
    r.close()


def test_batch_equals_one_at_a_time(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = RankedOr(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:60] + heavy_queries(ix.lens, 12)
    batch = r.run(qs, 10)
    for i, q in enumerate(qs):
        _assert_equal(r.run([q], 10), tuple(a[i:i + 1] for a in batch))
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_a_call_in_many_passes(device, small_corpus, kind, pass_pages):
    """query_or_pass_pages cuts a call into many passes (queries larger than the bound alone in a pass of their own):
    every pass writes its queries at their own place of the output."""
    ix = get_index(small_corpus, kind)
    r = RankedOr(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2) + [[], [0]]
    want = r.want(qs, 10)
    one = r.run(qs, 10)
    _assert_equal(one, want)
    device.set_option("query_or_pass_pages", pass_pages)
    _assert_equal(r.run(qs, 10), want)
    _assert_equal(r.run(qs[::-1], 10), tuple(a[::-1] for a in want))
    r.close()


def test_a_short_wand_handle_is_refused_before_any_launch(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = RankedOr(device, ix, kind)
    top = int(ix.docids.max())
    short = device.WandData(r.norm_lens[:top])  # num_docs == the largest docID
    with pytest.raises(device.DintError):
        r.qi.ranked_or_queries(r.fd, short, [[0]], k=10)
    lib = device._lib
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    assert lib.dint_ranked_or_queries(r.qi._h, r.fd._h, short._h, 10, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data,
                                      scores.ctypes.data, None, None) == DINT_ERR_ARG
    # docids may be null
    ok = device.WandData(r.norm_lens)
    assert lib.dint_ranked_or_queries(r.qi._h, r.fd._h, ok._h, 10, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data,
                                      scores.ctypes.data, None, None) == 0
    want = r.want([[0]], 10)
    assert counts[0] == want[0][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))
    # a freqs dictionary of another kind
    other = device.Dictionary(host.MULTI_PACKED, get_index(small_corpus, host.MULTI_PACKED).freqs_dict)
    with pytest.raises(device.DintError):
        r.qi.ranked_or_queries(other, ok, [[0]], k=10)
    short.close()
    ok.close()
    r.close()


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_reference_query_log_and_the_heavy_set(device, kind):
    """The reference's query log, term ids as they are, over the README-shaped collection, and its heaviest queries."""
    ix = ReadmeIndex(kind)
    r = RankedOr(device, ix, kind)
    qs = reference_queries(len(ix.lens))
    heavy = heavy_queries(ix.lens, 40)
    want = r.want(qs, 10)
    _assert_equal(r.run(qs, 10), want)
    assert int(want[0].sum()) > 4_000  # (at most 10 per query)
    _assert_equal(r.run(heavy, 10), r.want(heavy, 10))
    for i in range(0, len(qs), 29):
        _assert_equal(r.run([qs[i]], 10), tuple(a[i:i + 1] for a in want))
    r.close()


def test_ranked_or_ranked_and_or_and_interleaved_and_two_threads(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = RankedOr(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    want = r.want(qs, 10)
    want_ra = r.want_and(qs, 10)
    want_and = np.array([intersect(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    want_or = np.array([union(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    for _ in range(2):
        _assert_equal(r.run(qs, 10), want)
        _assert_equal(r.run_and(qs, 10), want_ra)
        assert np.array_equal(r.qi.or_queries(qs), want_or)
        assert np.array_equal(r.qi.and_queries(qs), want_and)
        assert np.array_equal(r.qi.or_queries_with_freqs(r.fd, qs)[0], want_or)
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            for _ in range(3):
                if which == 0:
                    _assert_equal(r.run(qs, 10), want)
                    assert np.array_equal(r.qi.or_queries(qs), want_or)
                else:
                    _assert_equal(r.run_and(qs, 10), want_ra)
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
