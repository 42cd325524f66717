"""The pruned ranked OR call under a wand handle with block maxima (dint_wand_data_set_block_max_weights, DESIGN.md
4d-maxscore "block maxima") on the GPU: the maxima built by dint_index_max_weights from the index itself; the answer
dint_ranked_or_queries' bit for bit; the blocks read the block-maxima model's (tests/blockmax.py), query by query, and never
more than the same handle read before it had block maxima. Then the contract on the block maxima: +inf reads exactly what
the term maxima read, halved ones only drop documents, a wrong count and a NaN are refused."""
import numpy as np
import pytest

import blockmax
import maxscore
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_query_fuzz import HandIndex
from test_gpu_ranked_or_maxscore import Pruned
from test_gpu_ranked_queries import _assert_equal
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
KS = (1, 10, 257)
PASSES = [None, 1, 2, 7]


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


class BlockPruned(Pruned):
    """Pruned with a third wand handle: term maxima and the block maxima the device built from the index."""

    def __init__(self, device, ix, kind, num_docs=None, norm_lens=None):
        super().__init__(device, ix, kind, num_docs=num_docs, norm_lens=norm_lens)
        dev_mtw, self.bmw = self.qi.max_weights(self.fd, self.wand, with_blocks=True)
        assert np.array_equal(dev_mtw.view(np.uint32), np.asarray(self.mtw, dtype=np.float32).view(np.uint32))
        self.bwand = device.WandData(self.norm_lens, max_term_weight=self.mtw)
        self.bwand.set_block_max_weights(self.bmw)
        self._models = {}

    def run_bm(self, qs, k):
        return self.qi.ranked_or_maxscore_queries(self.fd, self.bwand, qs, k=k)

    def models(self, qs, k):
        """(block-maxima model, term-maxima model) per query, computed once per (query, k)."""
        out = []
        for q in qs:
            key = (tuple(int(x) for x in q), k)
            if key not in self._models:
                self._models[key] = (blockmax.maxscore_blockmax(self.lists, q, self.norm_lens, self.mtw, self.bmw, self.num_docs, k),
                                     maxscore.maxscore(self.lists, q, self.norm_lens, self.mtw, self.num_docs, k))
            out.append(self._models[key])
        return out

    def check_bm(self, qs, k):
        """One batch and one query per call: == ranked_or (device); blocks read == the model's, per query, and <= the same
        index's under the handle without block maxima."""
        mods = self.models(qs, k)
        want = self.run(qs, k)
        got = self.run_bm(qs, k)
        _assert_equal(got[:3], want)
        assert got[3] == sum(b.blocks_read for b, _ in mods)
        assert got[3] <= self.run_ms(qs, k)[3]
        fewer = 0
        for i, (q, (b, t)) in enumerate(zip(qs, mods)):
            one = self.run_bm([q], k)
            _assert_equal(one[:3], tuple(a[i:i + 1] for a in want))
            before = self.run_ms([q], k)[3]
            print(f"k = {k}, query {i}: blocks read {one[3]} (model {b.blocks_read}), term maxima {before} (model {t.blocks_read})")
            assert one[3] == b.blocks_read
            assert before == t.blocks_read and one[3] <= before
            fewer += one[3] < before
        return fewer

    def close(self):
        super().close()
        self.bwand.close()


def small_sets(ix):
    """(judged by the models alone, tests/test_blockmax_cpu.py: some query reads strictly fewer blocks at every k of KS)"""
    return reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 10) + maxscore.mixed_queries(ix.lens, 20)


@pytest.fixture(scope="module")
def small(device, small_corpus):
    kind = host.SINGLE_PACKED
    r = BlockPruned(device, get_index(small_corpus, kind), kind)
    yield r
    r.close()


@pytest.fixture(scope="module")
def gain(device):
    lists, freqs, num_docs, nl, q = blockmax.certain_gain()
    h = HandIndex(device, host.SINGLE_PACKED, lists, freqs, num_docs, nl)

    class Ix:
        pass

    ix = Ix()
    ix.docids, ix.freqs, ix.lens, ix.bounds = h.docids, h.freqs, h.lens, h.bounds
    r = BlockPruned.__new__(BlockPruned)
    # (HandIndex has built the device side: the handles are taken over as Pruned would have made them)
    r.ix, r.num_docs, r.norm_lens, r.qi, r.fd, r.wand, r.lists = ix, num_docs, h.nl, h.qi, h.fd, h.wand, h.lists
    import ranked

    r.mtw = ranked.max_term_weights(h.docids, h.freqs, h.bounds, h.nl)
    r.mwand = device.WandData(h.nl, max_term_weight=r.mtw)
    dev_mtw, r.bmw = r.qi.max_weights(r.fd, r.wand, with_blocks=True)
    assert np.array_equal(dev_mtw.view(np.uint32), r.mtw.view(np.uint32))
    r.bwand = device.WandData(h.nl, max_term_weight=r.mtw)
    r.bwand.set_block_max_weights(r.bmw)
    r._models = {}
    yield r, q
    r.close()


@pytest.mark.parametrize("pass_pages", PASSES)
@pytest.mark.parametrize("k", KS)
def test_small_corpus_equal_to_ranked_or_and_the_model(device, small, k, pass_pages):
    qs = small_sets(small.ix)
    if pass_pages:
        device.set_option("query_or_pass_pages", pass_pages)
    assert small.check_bm(qs, k) >= 1  # (no vacuous comparison: the models say so in tests/test_blockmax_cpu.py)


@pytest.mark.parametrize("pass_pages", PASSES)
@pytest.mark.parametrize("k", KS)
def test_the_hand_made_case_where_the_gain_is_certain(device, gain, k, pass_pages):
    r, q = gain
    if pass_pages:
        device.set_option("query_or_pass_pages", pass_pages)
    r.check_bm([q, q[::-1], [1], [0]], k)
    if k == blockmax.GAIN_K:
        assert (r.run_ms([q], k)[3], r.run_bm([q], k)[3]) == (3 + 28, 3 + 1)


def test_block_maxima_of_infinity_read_what_the_term_maxima_read(device, small, gain):
    for r, qs in ((small, small_sets(small.ix)), (gain[0], [gain[1]])):
        w = device.WandData(r.norm_lens, max_term_weight=r.mtw)
        w.set_block_max_weights(np.full_like(r.bmw, np.inf))
        for k in KS:
            want = r.run(qs, k)
            _assert_equal(r.qi.ranked_or_maxscore_queries(r.fd, w, qs, k=k)[:3], want)
            for q in qs:
                assert r.qi.ranked_or_maxscore_queries(r.fd, w, [q], k=k)[3] == r.run_ms([q], k)[3]
        w.close()


def test_halved_block_maxima_only_drop_documents(device, small, gain):
    for r, qs in ((small, small_sets(small.ix)), (gain[0], [gain[1]])):
        w = device.WandData(r.norm_lens, max_term_weight=r.mtw)
        w.set_block_max_weights(r.bmw * np.float32(0.5))
        for k in KS:
            want = r.run(qs, k)
            got = r.qi.ranked_or_maxscore_queries(r.fd, w, qs, k=k)
            for i, (q, (b, _)) in enumerate(zip(qs, r.models(qs, k))):
                maxscore.assert_degraded(got[0][i], got[1][i], got[2][i], b, int(want[0][i]))
        w.close()


def test_a_wrong_block_count_and_a_nan_are_refused(device, small):
    r = small
    qs = small_sets(r.ix)[:20]
    before = r.run_bm(qs, 10)
    w = device.WandData(r.norm_lens, max_term_weight=r.mtw)
    for wrong in (r.bmw[:-1], np.concatenate([r.bmw, r.bmw[:1]]), r.bmw[:0]):
        w.set_block_max_weights(wrong)
        with pytest.raises(device.DintError) as e:
            r.qi.ranked_or_maxscore_queries(r.fd, w, qs, k=10)
        assert e.value.status == DINT_ERR_ARG
    w.close()
    # a NaN (or a negative value) is refused and the handle keeps the maxima it had
    for bad in (np.nan, -1.0):
        spoiled = r.bmw.copy()
        spoiled[spoiled.size // 2] = bad
        with pytest.raises(device.DintError) as e:
            r.bwand.set_block_max_weights(spoiled)
        assert e.value.status == DINT_ERR_ARG
        after = r.run_bm(qs, 10)
        _assert_equal(after[:3], before[:3])
        assert after[3] == before[3]
    # set again: the copy is replaced
    r.bwand.set_block_max_weights(np.full_like(r.bmw, np.inf))
    assert r.run_bm(qs, 10)[3] == r.run_ms(qs, 10)[3]
    r.bwand.set_block_max_weights(r.bmw)
    assert r.run_bm(qs, 10)[3] == before[3]
