"""MaxScore-pruned ranked OR queries on the GPU through the C ABI (dint_ranked_or_maxscore_queries): counts, BM25 scores and
docIDs bit-equal to dint_ranked_or_queries and to the models (tests/ranked_or.py, tests/maxscore.py), and the blocks read
equal to the pruned model's, query by query."""
import threading

import numpy as np
import pytest

import maxscore
from dint_amd import host
from or_union import union
from queries import ReadmeIndex, heavy_queries, intersect, reference_queries
from test_gpu_ranked_or_queries import RankedOr
from test_gpu_ranked_queries import _assert_equal, _hand_made
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


class Pruned(RankedOr):
    """RankedOr with a second wand handle that carries max_term_weight (host.wand_data's, as dint_create_wand_data writes it)."""

    def __init__(self, device, ix, kind, num_docs=None, norm_lens=None):
        super().__init__(device, ix, kind, num_docs=num_docs)
        if norm_lens is not None:
            self.norm_lens = norm_lens
            self.wand.close()
            self.wand = device.WandData(norm_lens)
        _, self.mtw = host.wand_data(self.sizes, ix.docids, ix.freqs, ix.lens)
        if norm_lens is not None:
            import ranked

            self.mtw = ranked.max_term_weights(ix.docids, ix.freqs, ix.bounds, norm_lens)
        self.mwand = device.WandData(self.norm_lens, max_term_weight=self.mtw)

    def run_ms(self, qs, k):
        return self.qi.ranked_or_maxscore_queries(self.fd, self.mwand, qs, k=k)

    def model(self, qs, k):
        return [maxscore.maxscore(self.lists, q, self.norm_lens, self.mtw, self.num_docs, k) for q in qs]

    def check(self, qs, k, blocks_each=False):
        """pruned == ranked_or (device) == the model; the total of blocks read == the model's (and query by query)."""
        got = self.run_ms(qs, k)
        want = self.want(qs, k)
        _assert_equal(got[:3], want)
        _assert_equal(self.run(qs, k), want)
        mod = self.model(qs, k)
        assert got[3] == sum(m.blocks_read for m in mod)
        if blocks_each:
            for q, m in zip(qs, mod):
                one = self.run_ms([q], k)
                assert one[3] == m.blocks_read
        return got, mod

    def close(self):
        super().close()
        self.mwand.close()


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_equal_to_ranked_or_and_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Pruned(device, ix, kind)
    qs = reference_queries(len(ix.lens))[::2] + heavy_queries(ix.lens, 40) + maxscore.mixed_queries(ix.lens, 40)
    for k in (10, 1, 1000):
        r.check(qs, k)
    r.close()


def test_blocks_read_query_by_query_and_below_or_freq(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    mixed = maxscore.mixed_queries(ix.lens, 40)
    qs = reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 10) + mixed
    r.check(qs, 10, blocks_each=True)
    got, mod = r.check(mixed, 10)
    or_blocks = r.qi.or_queries_with_freqs(r.fd, mixed)[2]
    assert or_blocks == sum(m.all_blocks for m in mod)
    assert got[3] < or_blocks
    r.close()


def test_edges(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    longest = int(np.argmax(ix.lens))
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    small = int(np.flatnonzero((ix.lens >= 1) & (ix.lens < 5))[0])
    qs = [[], [mid], [longest], [mid, mid], [mid, longest], [longest, mid, longest], [small], [small, small, mid]]
    got, _ = r.check(qs, 10, blocks_each=True)
    assert got[0][0] == 0 and (got[1][0] == 0).all() and (got[2][0] == 0xFFFFFFFF).all()
    assert got[0][6] == ix.lens[small]
    big, _ = r.check([[mid], [small, mid]], 1000)
    assert int(big[0][1]) == union(ix.docids, ix.bounds, [small, mid])
    r.check(qs, 1)
    r.close()


def test_disjoint_subset_clamped_idf_and_ties(device):
    """tests/test_gpu_ranked_or_queries.py's hand-made index: disjoint lists, subsets, the clamped idf, equal norm_lens and
    freqs, so that scores tie across the k-th place."""
    kind = host.MULTI_PACKED
    ix = _hand_made(device, kind)
    r = Pruned(device, ix, kind, num_docs=9000, norm_lens=np.ones(9000, dtype=np.float32))
    qs = [[0, 1], [1, 0], [3], [3, 4], [4, 3], [2, 4], [0, 2], [4], [2, 3, 4], [0, 1, 4]]
    for k in (10, 1, 1000):
        r.check(qs, k, blocks_each=k == 10)
    r.close()


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_reference_query_log_and_the_heavy_set(device, kind):
    ix = ReadmeIndex(kind)
    r = Pruned(device, ix, kind)
    qs = reference_queries(len(ix.lens))
    got, _ = r.check(qs, 10)
    r.check(heavy_queries(ix.lens, 40), 10)
    r.check(maxscore.mixed_queries(ix.lens, 40), 10)
    for i in range(0, len(qs), 37):
        one = r.run_ms([qs[i]], 10)
        _assert_equal(one[:3], tuple(a[i:i + 1] for a in got[:3]))
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:100] + heavy_queries(ix.lens, 20, seed=2) + maxscore.mixed_queries(ix.lens, 20) + [[], [0]]
    one = r.run_ms(qs, 10)
    device.set_option("query_or_pass_pages", pass_pages)
    got, _ = r.check(qs, 10)
    _assert_equal(got[:3], one[:3])
    assert got[3] == one[3]
    rev = r.run_ms(qs[::-1], 10)
    _assert_equal(rev[:3], tuple(a[::-1] for a in one[:3]))
    r.close()


def test_batch_equals_one_at_a_time(device, small_corpus):
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 8) + maxscore.mixed_queries(ix.lens, 12)
    batch = r.run_ms(qs, 10)
    total = 0
    for i, q in enumerate(qs):
        one = r.run_ms([q], 10)
        _assert_equal(one[:3], tuple(a[i:i + 1] for a in batch[:3]))
        total += one[3]
    assert total == batch[3]
    r.close()


def test_interleaved_with_ranked_or_and_or_on_two_threads(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:60] + heavy_queries(ix.lens, 8) + maxscore.mixed_queries(ix.lens, 12)
    want = r.want(qs, 10)
    blocks = sum(m.blocks_read for m in r.model(qs, 10))
    want_and = np.array([intersect(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    want_or = np.array([union(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            for _ in range(3):
                if which == 0:
                    got = r.run_ms(qs, 10)
                    _assert_equal(got[:3], want)
                    assert got[3] == blocks
                    assert np.array_equal(r.qi.or_queries(qs), want_or)
                else:
                    _assert_equal(r.run(qs, 10), want)
                    assert np.array_equal(r.qi.and_queries(qs), want_and)
                    got = r.run_ms(qs[::-1], 10)
                    _assert_equal(got[:3], tuple(a[::-1] for a in want))
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    r.close()


def test_refused_before_any_launch(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    lib = device._lib
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    with pytest.raises(device.DintError):  # a handle without maxima
        r.qi.ranked_or_maxscore_queries(r.fd, r.wand, [[mid]], k=10)
    few = device.WandData(r.norm_lens, max_term_weight=r.mtw[:-1])  # one list short
    with pytest.raises(device.DintError):
        r.qi.ranked_or_maxscore_queries(r.fd, few, [[mid]], k=10)
    top = int(ix.docids.max())
    short = device.WandData(r.norm_lens[:top], max_term_weight=r.mtw)  # num_docs == the largest docID
    with pytest.raises(device.DintError):
        r.qi.ranked_or_maxscore_queries(r.fd, short, [[mid]], k=10)
    with pytest.raises(device.DintError):
        r.run_ms([[len(ix.lens)]], 10)
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            r.run_ms([[mid]], bad_k)
    import ctypes as C

    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    terms = np.array([mid], dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(7)
    for w in (r.wand, few, short):
        assert lib.dint_ranked_or_maxscore_queries(r.qi._h, r.fd._h, w._h, 10, terms.ctypes.data, offs.ctypes.data, 1,
                                                   counts.ctypes.data, scores.ctypes.data, None, C.byref(blocks), None) == DINT_ERR_ARG
    # docids and blocks_read may be null
    assert lib.dint_ranked_or_maxscore_queries(r.qi._h, r.fd._h, r.mwand._h, 10, terms.ctypes.data, offs.ctypes.data, 1,
                                               counts.ctypes.data, scores.ctypes.data, None, None, None) == 0
    want = r.want([[mid]], 10)
    assert counts[0] == want[0][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))
    few.close()
    short.close()
    r.close()
