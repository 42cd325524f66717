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
    # a NaN or negative maximum, anywhere in the array: refused before the device is looked for (no std::sort over NaNs later)
    for bad in (np.nan, -np.nan, -1.0, -np.inf, -1e-45):
        for at in range(3):
            mw = np.array([0.5, 0.25, 1.0], dtype=np.float32)
            mw[at] = bad
            out = C.c_void_p(8)
            assert create(0, nl.ctypes.data, 4, mw.ctypes.data, 3, C.byref(out)) == DINT_ERR_ARG
            assert not out.value
    assert create(0, None, 0, np.array([np.nan], dtype=np.float32).ctypes.data, 1, C.byref(out)) == DINT_ERR_ARG


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


# ---------------------------------------------------------------------------------------------------------------
# the query fuzz plan (tests/test_gpu_query_fuzz.py's run_query_case) replayed on the model: the draws are the GPU test's
# own (tests/query_fuzz_draws.py). The floors are conditions of the plan: thin the plan or the mix until the pruned
# path idles and this test fails, whatever the device does.
# ---------------------------------------------------------------------------------------------------------------
import fuzz_streams as F  # noqa: E402
from query_fuzz_draws import draw_case  # noqa: E402
from test_fuzz_cpu import GOLDEN, QUERY  # noqa: E402

PLAN_FLOORS = {"non_empty_n": 250, "fewer_blocks": 200, "kth_is_theta": 200, "theta_zero": 100}
CASE_FLOOR_NON_EMPTY_N = 5


def plan_case_stats(case):
    """One case of the plan through the model, every (query, k) bit for bit against ranked_or -> its counts."""
    _, _, X = F.build_query_case(case)
    _, qs, nl, ks = draw_case(case[0], X)
    num_docs = int(X.docids.max()) + 1
    mod = Model(X.docids, X.freqs, X.bounds, num_docs=num_docs, norm_lens=nl)
    st = dict.fromkeys(("pairs", "pruned", *PLAN_FLOORS), 0)
    for k in ks:
        for q in qs:
            got = mod.check(q, k)
            n_terms = np.unique(np.asarray(q, dtype=np.int64)).size
            st["pairs"] += 1
            st["pruned"] += got.candidates.size < got.union.size
            st["non_empty_n"] += got.n_essential < n_terms
            st["fewer_blocks"] += got.blocks_read < got.all_blocks
            st["kth_is_theta"] += int(got.count == k and np.float32(got.theta) == got.scores[k - 1])
            st["theta_zero"] += n_terms > 0 and got.union.size > 0 and got.theta == 0.0
    return st


@pytest.fixture(scope="module")
def plan_stats():
    return {}


@pytest.mark.parametrize("case", QUERY, ids=lambda c: f"seed{c[0]}")
def test_the_fuzz_plan_case_on_the_model(case, plan_stats):
    assert str(case[0]) in GOLDEN["query"]
    st = plan_case_stats(case)
    print(f"seed {case[0]}: {st}")
    assert st["pairs"] == 2 * 60
    assert st["non_empty_n"] >= CASE_FLOOR_NON_EMPTY_N, st
    plan_stats[case[0]] = st


def test_the_fuzz_plan_drives_the_pruning(plan_stats):
    """Over the whole plan (measured when the floors were set: 1440 pairs, 1151 with a pruned document, 343 with a non-empty
    N, 307 reading fewer blocks, 295 with the k-th score equal to theta, 186 with theta 0)."""
    for case in QUERY:  # (a run of this test alone)
        if case[0] not in plan_stats:
            plan_stats[case[0]] = plan_case_stats(case)
    total = {key: sum(st[key] for st in plan_stats.values()) for key in next(iter(plan_stats.values()))}
    print(f"plan: {total}")
    assert total["pairs"] == 120 * len(QUERY)
    for key, floor in PLAN_FLOORS.items():
        assert total[key] >= floor, (key, total)


# ---------------------------------------------------------------------------------------------------------------
# the hand-made edges (tests/maxscore_edges.py): the model against what every query does by construction
# ---------------------------------------------------------------------------------------------------------------
import maxscore_edges as E  # noqa: E402


def _check_spec(spec):
    mod = Model(spec.docids, spec.all_freqs, spec.bounds, num_docs=spec.num_docs, norm_lens=spec.nl)
    out = []
    for q in spec.queries:
        mod.check(q.terms, q.k)
        out.append(spec.check_model(q))
    return out


@pytest.mark.parametrize("k,equal", E.LENGTH_CASES, ids=lambda v: str(v))
def test_list_lengths_on_k(k, equal):
    out = _check_spec(E.lengths_on_k(k, equal))
    assert out[0].n_essential == 1 and out[0].blocks_read < out[0].all_blocks  # (the rare seed alone is essential)


def test_seed_ties_go_to_the_smaller_term_id():
    spec = E.seed_ties()
    out = _check_spec(spec)
    # the two choices differ where they can be seen: theta, and with it the blocks read
    assert out[0].theta > out[2].theta and out[0].blocks_read < out[2].blocks_read
    assert out[0].blocks_read == out[1].blocks_read and out[2].blocks_read == out[3].blocks_read


def test_a_seed_with_theta_zero_prunes_nothing_and_counts_the_zero_score():
    spec = E.zero_theta()
    out = _check_spec(spec)
    assert [m.theta == 0.0 for m in out] == [True] * 5 + [False]
    assert out[3].count == 256 and out[3].scores[255] == 0.0 and out[3].ids[255] == spec.zero_doc


def test_a_subnormal_theta():
    out = _check_spec(E.subnormal_theta())
    tiny = float(np.finfo(np.float32).tiny)
    assert sum(0.0 < m.theta < tiny for m in out) >= 5, [m.theta for m in out]


def test_claim_geometry():
    out = _check_spec(E.claim_geometry())
    assert all(m.n_essential < len(set(q.terms)) for m, q in zip(out, E.claim_geometry().queries))


# ---------------------------------------------------------------------------------------------------------------
# maxima other than the exact ones, on the model: any upper bounds give ranked_or's answer (mod.check asserts it) and
# +inf reads every block; under-estimates only drop documents (maxscore.assert_degraded), and do drop some
# ---------------------------------------------------------------------------------------------------------------
def _maxima_case(which, request):
    if which == "small_corpus":
        ix = get_index(request.getfixturevalue(which), host.SINGLE_PACKED)
        mod = _model(ix)
        qs = reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 10) + maxscore.mixed_queries(ix.lens, 20)
        return mod, qs, (10, 257)
    case = QUERY[which]
    _, _, X = F.build_query_case(case)
    _, qs, nl, ks = draw_case(case[0], X)
    return Model(X.docids, X.freqs, X.bounds, num_docs=int(X.docids.max()) + 1, norm_lens=nl), qs, (10, ks[0])


@pytest.mark.parametrize("which", list(E.MAXIMA_FUZZ_CASES) + ["small_corpus"], ids=str)
def test_maxima_other_than_the_exact_ones_on_the_model(which, request):
    mod, qs, ks = _maxima_case(which, request)
    exact = mod.mtw
    for k in ks:
        want = [ranked_or.ranked_or(mod.lists, q, mod.nl, mod.num_docs, k) for q in qs]
        for name, mtw in E.upper_bounds(exact).items():
            mod.mtw = mtw
            for q in qs:
                got = mod.check(q, k)
                if name == "inf":
                    assert got.blocks_read == got.all_blocks and got.n_essential == np.unique(np.asarray(q, dtype=np.int64)).size
        for name, mtw in E.under_estimates(exact).items():
            mod.mtw = mtw
            differ = 0
            for q, w in zip(qs, want):
                got = maxscore.maxscore(mod.lists, q, mod.nl, mtw, mod.num_docs, k)
                maxscore.assert_degraded(got.count, got.scores, got.ids, got, int(w[0]))
                assert got.blocks_read <= got.all_blocks
                differ += not (got.count == w[0] and np.array_equal(got.ids, w[2]))
            print(f"{which}, k = {k}, {name}: {differ} of {len(qs)} answers differ from ranked_or's")
            if name == "zeros":
                assert differ > 0, "the under-estimates do drop documents here"
    mod.mtw = exact
