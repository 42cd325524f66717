"""Block maxima without a GPU: the model of dint_index_max_weights (tests/blockmax.py) against ranked.max_term_weights and
dinth_wand_data bit for bit, and the model of the pruned call under block maxima against the ranked-OR model bit for bit and
against the term-maxima model (tests/maxscore.py) block for block: never more blocks, and strictly fewer somewhere in every
query set the GPU tests use."""
import ctypes as C
import os

import numpy as np
import pytest

import blockmax
import maxscore
import ranked
import ranked_or
from dint_amd import host
from queries import ReadmeIndex, heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1
NEW = ("dint_index_max_weights", "dint_wand_data_set_block_max_weights")
CORPORA = ["small_corpus", "dense_corpus", "sparse_corpus"]


def test_the_entries_are_exported_and_listed():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    for name in NEW:
        assert hasattr(lib, name)
        assert name in device.ABI_SYMBOLS
    assert hasattr(device.QueryIndex, "max_weights") and hasattr(device.WandData, "set_block_max_weights")
    assert device.abi_version() == 6
    assert os.path.exists(os.path.join(ROOT, "dint_amd", "bin", "dint_index_wand_data"))


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments are refused first)
    out = np.zeros(4, dtype=np.float32)
    for qi, fd, wd in ((None, fake, fake), (fake, None, fake), (fake, fake, None), (None, None, None)):
        assert lib.dint_index_max_weights(qi, fd, wd, out.ctypes.data, None, None) == DINT_ERR_ARG
    setter = lib.dint_wand_data_set_block_max_weights
    assert setter(None, out.ctypes.data, 4) == DINT_ERR_ARG
    assert setter(fake, None, 4) == DINT_ERR_ARG
    # a NaN or negative value anywhere: refused before the handle or the device is touched
    for bad in (np.nan, -np.nan, -1.0, -np.inf, -1e-45):
        for at in range(3):
            bm = np.array([0.5, np.inf, np.finfo(np.float32).max], dtype=np.float32)
            bm[at] = bad
            assert setter(fake, bm.ctypes.data, 3) == DINT_ERR_ARG


class Model:
    def __init__(self, docids, freqs, bounds, lens, num_docs=None, norm_lens=None):
        self.num_docs = num_docs or int(docids.max()) + 1
        self.nl = norm_lens if norm_lens is not None else ranked.norm_lens(host.sizes_from_postings(docids, freqs, self.num_docs))
        self.mtw = ranked.max_term_weights(docids, freqs, bounds, self.nl)
        self.bmw = blockmax.block_max_weights(docids, freqs, bounds, self.nl)
        self.lists = ranked.BuilderLists(docids, freqs, bounds)
        self.lens = lens

    def both(self, q, k):
        """(the block-maxima model, the term-maxima model), the first held to ranked_or bit for bit and to <= the second's blocks."""
        got = blockmax.maxscore_blockmax(self.lists, q, self.nl, self.mtw, self.bmw, self.num_docs, k)
        term = maxscore.maxscore(self.lists, q, self.nl, self.mtw, self.num_docs, k)
        want = ranked_or.ranked_or(self.lists, q, self.nl, self.num_docs, k)
        assert got.count == want[0]
        assert np.array_equal(got.scores.view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(got.ids, want[2])
        assert got.theta == term.theta and got.n_essential == term.n_essential
        assert got.blocks_read <= term.blocks_read <= term.all_blocks
        assert np.isin(got.candidates, term.candidates).all()
        return got, term


def query_sets(lens, n=30):
    """The three sets of the pruned call's tests: the reference log, the heavy set and the mixed set."""
    return {"log": reference_queries(len(lens))[::3], "heavy": heavy_queries(lens, n), "mixed": maxscore.mixed_queries(lens, n)}


@pytest.mark.parametrize("corpus_name", CORPORA)
def test_block_maxima_give_the_term_maxima_and_dinth_wand_data(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    num_docs = int(ix.docids.max()) + 1
    sizes = host.sizes_from_postings(ix.docids, ix.freqs, num_docs)
    nl, mtw = host.wand_data(sizes, ix.docids, ix.freqs, ix.lens)
    assert np.array_equal(nl.view(np.uint32), ranked.norm_lens(sizes).view(np.uint32))
    bmw = blockmax.block_max_weights(ix.docids, ix.freqs, ix.bounds, nl)
    assert bmw.size == int(((ix.lens.astype(np.int64) + 255) // 256).sum()) and (bmw > 0).all()
    of_blocks = blockmax.term_maxima_of_blocks(bmw, ix.bounds)
    assert np.array_equal(of_blocks.view(np.uint32), ranked.max_term_weights(ix.docids, ix.freqs, ix.bounds, nl).view(np.uint32))
    assert np.array_equal(of_blocks.view(np.uint32), mtw.view(np.uint32))


def test_a_zero_length_and_a_nan_never_enter_a_maximum():
    """norm_len 0 under freq 0 (a wrapped freq) is 0 / 0: the host's std::max(max, score) from 0.0f keeps its maximum."""
    docids = np.array([0, 1, 2, 3], dtype=np.uint32)
    freqs = np.array([0, 3, 0, 0], dtype=np.uint32)
    nl = np.array([-1.0, 1.0, 1.0, -1.0], dtype=np.float32)  # (kd = 0 at -1: 0 / 0)
    bounds = np.array([0, 2, 4], dtype=np.uint64)
    bmw = blockmax.block_max_weights(docids, freqs, bounds, nl)
    assert bmw[0] == ranked.doc_term_weight(np.array([3]), np.array([1.0], dtype=np.float32))[0] and bmw[1] == 0.0
    assert not np.signbit(bmw[1])


@pytest.fixture(scope="module")
def fewer(request):
    return {}


@pytest.mark.parametrize("corpus_name", CORPORA)
def test_same_answer_never_more_blocks(request, corpus_name, fewer):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    mod = Model(ix.docids, ix.freqs, ix.bounds, ix.lens)
    for name, qs in query_sets(ix.lens).items():
        n = pairs = 0
        for k in (1, 10, 1000):
            for q in (qs if k != 1000 else qs[::3]):
                got, term = mod.both(q, k)
                pairs += 1
                n += got.blocks_read < term.blocks_read
        fewer[(corpus_name, name)] = (n, pairs)
        print(f"{corpus_name}, {name}: {n} of {pairs} (query, k) pairs read strictly fewer blocks under block maxima")


def gpu_sets(small_corpus):
    """What tests/test_gpu_ranked_or_blockmax.py runs on the small corpus (one set: its slices of the three)."""
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    return ix, reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 10) + maxscore.mixed_queries(ix.lens, 20)


def test_the_gpu_comparisons_are_not_vacuous(small_corpus):
    """Every (set, k) the GPU test compares has a query that reads strictly fewer blocks under block maxima, by the models."""
    ix, qs = gpu_sets(small_corpus)
    mod = Model(ix.docids, ix.freqs, ix.bounds, ix.lens)
    for k in (1, 10, 257):
        n = sum(g.blocks_read < t.blocks_read for g, t in (mod.both(q, k) for q in qs))
        print(f"small corpus, the GPU test's set, k = {k}: {n} of {len(qs)} queries read strictly fewer blocks")
        assert n >= 1, k


def test_the_hand_made_case_where_the_gain_is_certain():
    lists, freqs, num_docs, nl, q = blockmax.certain_gain()
    lens = np.array([x.size for x in lists], dtype=np.uint32)
    bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    mod = Model(np.concatenate(lists), np.concatenate(freqs), bounds, lens, num_docs=num_docs, norm_lens=nl)
    got, term = mod.both(q, blockmax.GAIN_K)
    seed, seed_f = lists[0], freqs[0]
    assert got.n_essential == 1                                             # the long list's term maximum keeps it in N
    assert np.float32(got.theta) == (ranked.query_term_weight(1, 600, num_docs) * ranked.doc_term_weight(np.array([50]), nl[:1]))[0]
    assert np.array_equal(term.candidates, seed)                            # the term bound keeps every candidate alive
    lo, hi = lists[1][256 * blockmax.GAIN_BLOCK - 1], lists[1][256 * blockmax.GAIN_BLOCK + 255]
    inside = seed[(seed > lo) & (seed <= hi)]
    assert inside.size == 23 and np.isin(seed[seed_f == 50], inside).all()
    assert np.array_equal(got.candidates, inside)                           # the block bound: only where the one posting is
    assert (term.blocks_read, got.blocks_read) == (3 + 28, 3 + 1)
    for k in (1, 257):
        mod.both(q, k)
