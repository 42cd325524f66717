"""MaxScore-pruned ranked OR queries without a GPU: the C ABI's new entries and their argument checks, and the model of the
pruned call (tests/maxscore.py) against the ranked-OR model (tests/ranked_or.py) bit for bit, with the pruning argument
checked on every document: nothing pruned scores as much as the threshold."""
import ctypes as C
import os

import numpy as np
import pytest

import maxscore
import ranked
import ranked_or
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1
NEW = ("dint_wand_data_create_with_max_weights", "dint_ranked_or_maxscore_queries")


def test_the_entries_are_exported_and_listed():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    for name in NEW:
        assert hasattr(lib, name)
        assert name in device.ABI_SYMBOLS
    assert hasattr(device.QueryIndex, "ranked_or_maxscore_queries")
    assert device.abi_version() == 6
    assert not [o for o in device.OPTIONS if "maxscore" in o]


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    ids = np.zeros(2048, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64()
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and the bad k are refused first)
    call = lib.dint_ranked_or_maxscore_queries
    for qi, fd, w, k in ((None, fake, fake, 10), (fake, None, fake, 10), (fake, fake, None, 10), (None, None, None, 10),
                         (fake, fake, fake, 0), (fake, fake, fake, 1025), (fake, fake, fake, 1 << 31)):
        assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, 1, counts.ctypes.data, scores.ctypes.data,
                    ids.ctypes.data, C.byref(blocks), None) == DINT_ERR_ARG
    assert call(None, None, None, 10, None, None, 0, None, None, None, None, None) == DINT_ERR_ARG
    nl = np.ones(4, dtype=np.float32)
    out = C.c_void_p()
    create = lib.dint_wand_data_create_with_max_weights
    assert create(0, nl.ctypes.data, 4, None, 3, C.byref(out)) == DINT_ERR_ARG  # maxima of 3 lists, none given
    assert create(0, nl.ctypes.data, 4, nl.ctypes.data, 3, None) == DINT_ERR_ARG
    assert not out.value


class Model:
    def __init__(self, docids, freqs, bounds, num_docs=None, norm_lens=None):
        self.num_docs = num_docs or int(docids.max()) + 1
        self.nl = norm_lens if norm_lens is not None else ranked.norm_lens(host.sizes_from_postings(docids, freqs, self.num_docs))
        self.mtw = ranked.max_term_weights(docids, freqs, bounds, self.nl)
        self.lists = ranked.BuilderLists(docids, freqs, bounds)

    def check(self, q, k):
        """The pruned model == ranked_or bit for bit, and every document left out scores below theta -> the result."""
        got = maxscore.maxscore(self.lists, q, self.nl, self.mtw, self.num_docs, k)
        want = ranked_or.ranked_or(self.lists, q, self.nl, self.num_docs, k)
        assert got.count == want[0]
        assert np.array_equal(got.scores.view(np.uint32), want[1].view(np.uint32))
        assert np.array_equal(got.ids, want[2])
        out = ~np.isin(got.union, got.candidates)
        assert (got.union_scores[out] < np.float32(got.theta)).all()
        assert got.blocks_read <= got.all_blocks
        return got


def _model(ix):
    return Model(ix.docids, ix.freqs, ix.bounds)


@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_the_model_is_ranked_or_bit_for_bit(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    mod = _model(ix)
    log = reference_queries(len(ix.lens))
    sets = {"log": log[::3], "heavy": heavy_queries(ix.lens, 30), "mixed": maxscore.mixed_queries(ix.lens, 30)}
    pruned = 0
    for k in (1, 10, 1000):
        for name, qs in sets.items():
            for q in (qs if k != 1000 else qs[::3]):
                got = mod.check(q, k)
                pruned += got.union.size - got.candidates.size
    assert pruned > 0


def test_the_mixed_set_reads_fewer_blocks(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    mod = _model(ix)
    qs = maxscore.mixed_queries(ix.lens, 40)
    read = all_blocks = 0
    for q in qs:
        got = mod.check(q, 10)
        read += got.blocks_read
        all_blocks += got.all_blocks
    assert read < all_blocks


def test_ties_with_theta_are_kept_in_docid_order():
    """Every norm_len 1 and every freq 1: a = 1000..1099 and 20000..20099, b = 0..9999. Query [a, b], k = 150: the seed
    is a and theta its common addend; a's first 100 documents are in b too and score more; the next 50 are a's
    documents outside b, which score exactly theta: they are kept, by ascending docID. b's documents outside a score less
    and are never candidates; b's blocks are read only where a's documents fall."""
    a = np.concatenate([np.arange(1000, 1100), np.arange(20000, 20100)]).astype(np.uint32)
    b = np.arange(0, 10000, dtype=np.uint32)
    docids = np.concatenate([a, b])
    freqs = np.ones(docids.size, dtype=np.uint32)
    bounds = np.array([0, a.size, a.size + b.size], dtype=np.uint64)
    num_docs = 20100
    mod = Model(docids, freqs, bounds, num_docs=num_docs, norm_lens=np.ones(num_docs, dtype=np.float32))
    got = mod.check([0, 1], 150)
    assert got.n_essential == 1
    theta = np.float32(got.theta)
    assert np.array_equal(got.ids[:100], np.arange(1000, 1100)) and (got.scores[:100] > theta).all()
    assert np.array_equal(got.ids[100:150], np.arange(20000, 20050)) and (got.scores[100:150] == theta).all()
    assert got.blocks_read == 1 + 2  # a's one block, b's blocks of 768..1023 and 1024..1279
    # one term alone: every candidate's bound is its own addend; the 150th ties with 50 more, and the tie is kept
    one = mod.check([0], 150)
    assert np.float32(one.theta) == one.scores[149] and one.candidates.size == 200
    for k in (1, 10, 100, 101, 200):
        mod.check([0, 1], k)
        mod.check([1, 0, 1], k)
