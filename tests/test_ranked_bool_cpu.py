"""Ranked boolean queries without a GPU: the model (tests/ranked_bool.py) against ranked.ranked_and where the optional and
excluded clauses are empty, against its float64 form and against plain set arithmetic; the new entry in the header and the
binding; and the inputs of tests/test_gpu_ranked_bool.py shown not to be vacuous (optional terms reorder a top k, exclusions
take documents out of one, empty a query, optional lists end before a match, a heavy query reads a part of its blocks)."""
import os

import numpy as np
import pytest

import ranked
import ranked_bool as RB
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPORA = ["small_corpus", "dense_corpus", "sparse_corpus"]


def _setup(ix):
    num_docs = int(ix.docids.max()) + 1
    nl = ranked.norm_lens(host.sizes_from_postings(ix.docids, ix.freqs, num_docs))
    return ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds), nl, num_docs


def test_the_entry_is_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert "int dint_ranked_bool_queries(" in header
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "dint_ranked_bool_queries" in device.ABI_SYMBOLS and hasattr(device._lib, "dint_ranked_bool_queries")
    assert hasattr(device.QueryIndex, "ranked_bool_queries")


def test_argument_errors_need_no_device():
    import ctypes as C

    from dint_amd import device

    call = device._lib.dint_ranked_bool_queries
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for qi, fd, w, k in ((None, fake, fake, 10), (fake, None, fake, 10), (fake, fake, None, 10), (fake, fake, fake, 0),
                         (fake, fake, fake, 1025)):
        assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, None, None, None, 1, counts.ctypes.data, None,
                    scores.ctypes.data, None, None, None) == -1


@pytest.mark.parametrize("corpus_name", CORPORA)
def test_empty_optional_and_excluded_clauses_are_ranked_and(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    qs = reference_queries(len(ix.lens))
    matched = 0
    for q in qs:
        for k in (10, 1000):
            n, m, sc, ids, _ = RB.ranked_bool(lists, q, [], [], nl, num_docs, k)
            want = ranked.ranked_and(lists, q, nl, num_docs, k)
            assert n == want[0] and np.array_equal(sc.view(np.uint32), want[1].view(np.uint32)) and np.array_equal(ids, want[2])
            assert n == min(k, m)
        matched += m
    assert matched > 500


def test_no_required_term_selects_nothing(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    for q in reference_queries(len(ix.lens))[:50] + [[]]:
        n, m, sc, ids, blocks = RB.ranked_bool(lists, [], q, [], nl, num_docs, 10)
        assert (n, m, blocks) == (0, 0, 0) and (sc == 0).all() and (ids == 0xFFFFFFFF).all()
        assert RB.ranked_bool(lists, [], q, q, nl, num_docs, 10)[:2] == (0, 0)


def test_model_against_float64_and_set_arithmetic(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    must, should, exclude = RB.gpu_batch_clauses(ix.lens)
    checked = with_optional = 0
    for mu, sh, ex in list(zip(must, should, exclude))[::3]:
        want = None
        for t in mu:
            d = lists.postings(t)[0]
            want = d if want is None else np.intersect1d(want, d)
        for t in ex:
            want = np.setdiff1d(want, lists.postings(t)[0])
        n_all = 0 if want is None else want.size
        n, m, sc, ids, _ = RB.ranked_bool(lists, mu, sh, ex, nl, num_docs, max(1, n_all))
        assert m == n_all == n
        if n == 0:
            continue
        f64 = RB.ranked_bool_f64(lists, mu, sh, ex, nl, num_docs)
        assert set(ids[:n].tolist()) == set(f64) == set(want.tolist())
        terms = len(mu) + len(sh)
        for s, d in zip(sc[:n].tolist(), ids[:n].tolist()):
            assert s > 0 and abs(s - f64[d]) <= 1e-6 * f64[d] * max(4, 2 * terms)  # (tests/test_ranked_cpu.py's tolerance)
        assert (np.diff(sc[:n]) <= 0).all()
        ties = np.diff(sc[:n]) == 0
        assert (np.diff(ids[:n].astype(np.int64))[ties] > 0).all()
        checked += n
        with_optional += n if sh else 0
    assert checked > 5_000 and with_optional > 100


def test_multiplicities_and_shared_terms(small_corpus):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    big = np.argsort(-ix.lens.astype(np.int64), kind="stable")
    a, b, c = int(big[3]), int(big[1]), int(big[0])
    plain = RB.ranked_bool(lists, [a, b], [c], [], nl, num_docs, 10)
    twice = RB.ranked_bool(lists, [a, b], [c, c], [], nl, num_docs, 10)
    assert plain[1] == twice[1] > 10 and not np.array_equal(plain[2], twice[2])  # qf = 2 within the optional clause
    # a term in must and should is scored once in each phase: more than the required terms alone give
    both = RB.ranked_bool(lists, [a, b], [b], [], nl, num_docs, 10)
    alone = RB.ranked_bool(lists, [a, b], [], [], nl, num_docs, 10)
    assert both[1] == alone[1] and (both[2][:both[0]] > alone[2][:alone[0]]).all()
    # a term in must and not matches nothing
    assert RB.ranked_bool(lists, [a, b], [c], [b], nl, num_docs, 10)[:2] == (0, 0)


def test_the_gpu_inputs_are_not_vacuous(small_corpus):
    """What tests/test_gpu_ranked_bool.py's batch must exercise, counted on the model over its own inputs."""
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    must, should, exclude = RB.gpu_batch_clauses(ix.lens)
    reordered = lost = emptied = ends_before = 0
    for mu, sh, ex in zip(must, should, exclude):
        if not sh and not ex:
            continue
        n, m, _, ids, _ = RB.ranked_bool(lists, mu, sh, ex, nl, num_docs, 10)
        base = ranked.ranked_and(lists, mu, nl, num_docs, 10)
        kept = RB.ranked_bool(lists, mu, sh, [], nl, num_docs, 10)
        if not ex and n and not np.array_equal(ids, base[2]):
            reordered += 1
        if ex and np.setdiff1d(kept[3][:kept[0]], ids[:n]).size:
            lost += 1
        if ex and kept[1] > 0 and m == 0:
            emptied += 1
        if sh and m:
            every = RB.ranked_bool(lists, mu, sh, ex, nl, num_docs, max(1, m))[3][:m]
            if any(lists.postings(t)[0].size and int(lists.postings(t)[0][-1]) < int(every.max()) for t in sh):
                ends_before += 1
    print("reordered", reordered, "lost", lost, "emptied", emptied, "ends_before", ends_before)
    assert reordered >= 1 and lost >= 1 and emptied >= 1 and ends_before >= 1


def test_a_heavy_query_reads_a_part_of_its_blocks(small_corpus):
    """The floor of tests/test_gpu_ranked_bool.py's laziness test: no heavy query claims more blocks than its terms have, and
    the one that test runs (RB.laziest_heavy_query) claims strictly fewer."""
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    must, should, exclude = RB.split_clauses(heavy_queries(ix.lens, 40), ix.lens)
    for mu, sh, ex in zip(must, should, exclude):
        assert RB.ranked_bool(lists, mu, sh, ex, nl, num_docs, 10)[4] <= RB.all_blocks(ix.lens, mu, sh, ex)
    (mu, sh, ex), claimed, every = RB.laziest_heavy_query(lists, ix.lens, nl, num_docs)
    print("claimed", claimed, "of", every)
    assert sh and ex and 0 < claimed < every
