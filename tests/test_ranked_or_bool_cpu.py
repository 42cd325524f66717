"""Union-driven ranked boolean queries without a GPU: the model (tests/ranked_or_bool.py) against ranked_or.ranked_or where m <= 1
and nothing is excluded, against set intersection where m is the number of terms, against plain set arithmetic and its
float64 form, and — document by document — against the model of dint_score_documents; the new entry in the header and the
binding; and the inputs of tests/test_gpu_ranked_or_bool.py shown not to be vacuous on the three corpora (m = 2 changes a
top 10, an exclusion takes a document out of one, an excluded list is decoded in part, m and an exclusion each empty a query)."""
import os

import numpy as np
import pytest

import ranked
import ranked_or
import ranked_or_bool as ROB
import score_documents as S
from dint_amd import host
from maxscore import blocks_of
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPORA = ["small_corpus", "dense_corpus", "sparse_corpus"]


def _setup(ix):
    num_docs = int(ix.docids.max()) + 1
    nl = ranked.norm_lens(host.sizes_from_postings(ix.docids, ix.freqs, num_docs))
    return ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds), nl, num_docs


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_the_entry_is_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert "int dint_ranked_or_bool_queries(" in header
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "dint_ranked_or_bool_queries" in device.ABI_SYMBOLS and hasattr(device._lib, "dint_ranked_or_bool_queries")
    assert hasattr(device.QueryIndex, "ranked_or_bool_queries")


def test_argument_errors_need_no_device():
    import ctypes as C

    from dint_amd import device

    call = device._lib.dint_ranked_or_bool_queries
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for qi, fd, w, k in ((None, fake, fake, 10), (fake, None, fake, 10), (fake, fake, None, 10), (fake, fake, fake, 0),
                         (fake, fake, fake, 1025)):
        assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, None, None, 1, counts.ctypes.data, None,
                    scores.ctypes.data, None, None, None) == -1


@pytest.mark.parametrize("corpus_name", CORPORA)
def test_without_a_minimum_and_exclusions_it_is_ranked_or(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    matched = 0
    for q in reference_queries(len(ix.lens))[::10]:
        want = {k: ranked_or.ranked_or(lists, q, nl, num_docs, k) for k in (10, 1000)}
        for m in (None, 0, 1):
            ev = ROB.evaluate(lists, q, [], m, nl, num_docs)
            for k in (10, 1000):
                n, mt, sc, ids, blocks = ev.top(k)
                assert n == want[k][0] == min(k, mt) and np.array_equal(bits(sc), bits(want[k][1])) and np.array_equal(ids, want[k][2])
            assert blocks == sum(blocks_of(int(ix.lens[t])) for t in set(int(t) for t in q)) * (mt > 0)
        matched += mt
    assert matched > 500


def test_every_term_asked_for_is_the_intersection(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    checked = 0
    for q in reference_queries(len(ix.lens))[::3] + heavy_queries(ix.lens, 20):
        u = ROB.distinct(q)
        want = None
        for t in u:
            d = lists.postings(t)[0]
            want = d if want is None else np.intersect1d(want, d)
        ev = ROB.evaluate(lists, q, [], len(u), nl, num_docs)
        assert np.array_equal(ev.docs, want)
        assert ROB.evaluate(lists, q, [], len(u) + 1, nl, num_docs).top(10)[:2] == (0, 0)
        assert ROB.evaluate(lists, q, [], len(u) + 1, nl, num_docs).blocks == 0
        checked += want.size
    assert checked > 500


def test_model_against_set_arithmetic_float64_and_score_documents(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    should, exclude, mins = ROB.gpu_batch_clauses(ix.lens)
    checked = with_exclusion = with_min = 0
    for sh, ex, m in list(zip(should, exclude, mins))[::3]:
        ev = ROB.evaluate(lists, sh, ex, m, nl, num_docs)
        # plain set arithmetic
        held = {}
        for t in set(sh):
            for d in lists.postings(t)[0].tolist():
                held[d] = held.get(d, 0) + 1
        want = {d for d, n in held.items() if n >= max(1, m)}
        for t in ex:
            want -= set(lists.postings(t)[0].tolist())
        n, mt, sc, ids, _ = ev.top(max(1, len(want)))
        assert mt == len(want) == n and set(ids[:n].tolist()) == want
        if n == 0:
            continue
        f64 = ROB.ranked_or_bool_f64(lists, sh, ex, m, nl, num_docs)
        assert set(f64) == want
        for s, d in zip(sc[:n].tolist(), ids[:n].tolist()):
            assert s > 0 and abs(s - f64[d]) <= 1e-6 * f64[d] * max(4, 2 * len(sh))  # (tests/test_ranked_cpu.py's tolerance)
        assert (np.diff(sc[:n]) <= 0).all()
        ties = np.diff(sc[:n]) == 0
        assert (np.diff(ids[:n].astype(np.int64))[ties] > 0).all()
        # every returned score is dint_score_documents' score of that document for the optional terms
        top = ev.top(10)
        mod = S.model_batch(lists, [sh], [top[3][:top[0]]], nl, num_docs)[0]
        assert np.array_equal(bits(mod.scores), bits(top[2][:top[0]]))
        checked += n
        with_exclusion += n if ex else 0
        with_min += n if m >= 2 else 0
    assert checked > 5_000 and with_exclusion > 100 and with_min > 100


def test_random_lists_against_set_arithmetic():
    """Short random lists, so that every combination of m and exclusions has documents on both sides of it."""
    rng = np.random.default_rng(11)
    docids, freqs, bounds = [], [], [0]
    for i in range(12):  # (list 3: empty)
        d = np.unique(rng.integers(0, 400, 0 if i == 3 else int(rng.integers(1, 300)))).astype(np.uint32)
        docids.append(d), freqs.append(rng.integers(1, 6, d.size).astype(np.uint32)), bounds.append(bounds[-1] + d.size)
    lists = ranked.BuilderLists(np.concatenate(docids), np.concatenate(freqs), np.array(bounds))
    nl = (rng.random(400) * 2 + 0.1).astype(np.float32)
    seen = 0
    for _ in range(200):
        sh = rng.integers(0, 12, int(rng.integers(0, 6))).tolist()
        ex = rng.integers(0, 12, int(rng.integers(0, 3))).tolist()
        m = int(rng.integers(0, 5))
        held = {}
        for t in set(sh):
            for d in docids[t].tolist():
                held[d] = held.get(d, 0) + 1
        want = {d for d, n in held.items() if n >= max(1, m)} if max(1, m) <= len(set(sh)) else set()
        for t in ex:
            want -= set(docids[t].tolist())
        ev = ROB.evaluate(lists, sh, ex, m, nl, 400)
        assert set(ev.docs.tolist()) == want and ev.docs.size == len(want)
        assert set(ROB.ranked_or_bool_f64(lists, sh, ex, m, nl, 400)) == want
        seen += len(want)
    assert seen > 5_000


def test_multiplicities_and_shared_terms(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    big = np.argsort(-ix.lens.astype(np.int64), kind="stable")
    a, b, c = int(big[3]), int(big[1]), int(big[0])
    plain = ROB.ranked_or_bool(lists, [a, b], [], 2, nl, num_docs, 10)
    twice = ROB.ranked_or_bool(lists, [a, b, b], [], 2, nl, num_docs, 10)
    assert plain[1] == twice[1] > 10 and not np.array_equal(plain[2], twice[2])  # qf = 2 scores; m counts distinct terms
    assert ROB.ranked_or_bool(lists, [a, a], [], 2, nl, num_docs, 10)[:2] == (0, 0)
    # a term in both clauses matches nothing through its list; repeats in `not` are one term
    both = ROB.evaluate(lists, [a, b], [b, b], 1, nl, num_docs)
    assert np.array_equal(both.docs, np.setdiff1d(lists.postings(a)[0], lists.postings(b)[0])) and len(both.lazy) == 1
    # excluded terms never score: the survivors keep ranked_or's scores
    kept = ROB.evaluate(lists, [a, b], [c], 1, nl, num_docs)
    every = ROB.evaluate(lists, [a, b], [], 1, nl, num_docs)
    at = np.searchsorted(every.docs, kept.docs)
    assert 0 < kept.docs.size < every.docs.size and np.array_equal(bits(every.scores[at]), bits(kept.scores))


@pytest.mark.parametrize("corpus_name", CORPORA)
def test_the_gpu_inputs_are_not_vacuous(request, corpus_name):
    """What tests/test_gpu_ranked_or_bool.py's batch must exercise, counted on the model over its own inputs."""
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    should, exclude, mins = ROB.gpu_batch_clauses(ix.lens)
    reordered = lost = lazy = emptied_by_m = emptied_by_not = 0
    for sh, ex, m in zip(should, exclude, mins):
        ev = ROB.evaluate(lists, sh, ex, m, nl, num_docs)
        ids = ev.top(10)[3]
        if m >= 2:
            loose = ROB.evaluate(lists, sh, ex, 1, nl, num_docs)
            reordered += not np.array_equal(ids, loose.top(10)[3])
            emptied_by_m += loose.docs.size > 0 and ev.docs.size == 0
        if ex:
            kept = ROB.evaluate(lists, sh, [], m, nl, num_docs)
            top = kept.top(10)
            lost += np.setdiff1d(top[3][:top[0]], ids).size > 0
            emptied_by_not += kept.docs.size > 0 and ev.docs.size == 0
            lazy += any(claimed < every for _, claimed, every in ev.lazy)
    print(corpus_name, "reordered", reordered, "lost", lost, "lazy", lazy, "emptied by m", emptied_by_m, "by not", emptied_by_not)
    assert reordered >= 10 and lost >= 10 and lazy >= 10
    assert emptied_by_m >= 1 and emptied_by_not >= 1
