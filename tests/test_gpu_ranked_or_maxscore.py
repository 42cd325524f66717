"""MaxScore-pruned ranked OR queries on the GPU through the C ABI (dint_ranked_or_maxscore_queries): counts, BM25 scores and
docIDs bit-equal to dint_ranked_or_queries and to the models (tests/ranked_or.py, tests/maxscore.py), and the blocks read
equal to the pruned model's, query by query. Then the call's contract on its maxima (any upper bounds: the same answer;
under-estimates: documents dropped and nothing else; NaN and negative ones refused at creation), on two cases of the query
fuzz plan and a corpus, and the hand-made edges of tests/maxscore_edges.py: list lengths on k, the seed's ties, thresholds of
0.0 and of subnormal size, the geometry of the claims, and a handle reused across calls of different sizes."""
import threading

import numpy as np
import pytest

import fuzz_streams as F
import maxscore
import maxscore_edges as E
import ranked
import ranked_or
from dint_amd import host
from or_union import union
from queries import ReadmeIndex, heavy_queries, intersect, reference_queries
from query_fuzz_draws import draw_case
from test_gpu_query_fuzz import QUERY, HandIndex, assert_ranked, ranked_want
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


# ---------------------------------------------------------------------------------------------------------------
# maxima other than the exact ones (include/dint_hip.h: upper bounds give the same answer, smaller maxima may drop documents)
# ---------------------------------------------------------------------------------------------------------------
class FuzzIndex:
    """A case of the query fuzz plan with its own draws (tests/query_fuzz_draws.py): the fuzz dictionaries, decoder-legal
    lists of up to 80 pages, wrapped freqs, the case's norm_lens class, its 60 queries and its first k."""

    def __init__(self, device, case):
        Dd, Df, X = F.build_query_case(case)
        _, self.qs, self.norm_lens, self.ks = draw_case(case[0], X)
        self.qi = device.QueryIndex(device.Dictionary(Dd.kind, Dd.file), X.index, X.offsets)
        self.fd = device.Dictionary(Df.kind, Df.file)
        self.num_docs = int(X.docids.max()) + 1
        self.lists = ranked.BuilderLists(X.docids, X.freqs, X.bounds)
        self.mtw = ranked.max_term_weights(X.docids, X.freqs, X.bounds, self.norm_lens)

    def close(self):
        self.qi.close()


def _maxima_subject(device, which, request):
    if which == "small_corpus":
        ix = get_index(request.getfixturevalue(which), host.SINGLE_PACKED)
        r = Pruned(device, ix, host.SINGLE_PACKED)
        return r, reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 10) + maxscore.mixed_queries(ix.lens, 20), (10, 257)
    r = FuzzIndex(device, QUERY[which])
    return r, r.qs, (10, r.ks[0])


@pytest.mark.parametrize("which", list(E.MAXIMA_FUZZ_CASES) + ["small_corpus"], ids=str)
def test_maxima_that_are_upper_bounds_change_no_answer(device, request, which):
    """mtw * 1.5, all 1.0 (f / (f + kd) <= 1), all FLT_MAX and all +inf: ranked_or's answer bit for bit, the blocks read the
    model's under the same maxima; +inf leaves N empty, so every block of every distinct term is read."""
    r, qs, ks = _maxima_subject(device, which, request)
    for name, mtw in E.upper_bounds(r.mtw).items():
        wand = device.WandData(r.norm_lens, max_term_weight=mtw)
        for k in ks:
            want = ranked_want(ranked_or.ranked_or, r.lists, qs, r.norm_lens, r.num_docs, k)
            got = r.qi.ranked_or_maxscore_queries(r.fd, wand, qs, k=k)
            assert_ranked(got[:3], want, (which, name, k))
            mods = [maxscore.maxscore(r.lists, q, r.norm_lens, mtw, r.num_docs, k) for q in qs]
            assert got[3] == sum(m.blocks_read for m in mods), (which, name, k)
            if name == "inf":
                assert got[3] == sum(m.all_blocks for m in mods)
        wand.close()
    r.close()


@pytest.mark.parametrize("which", list(E.MAXIMA_FUZZ_CASES) + ["small_corpus"], ids=str)
def test_maxima_below_the_true_ones_only_drop_documents(device, request, which):
    """mtw * 0.5 and all zeros: DINT_OK, every (docID, score) returned a document of the union with its exact ranked_or
    score, in strict (score descending, docID ascending) order, no more of them than ranked_or returns, no more blocks
    than every block — and the model's answer and blocks exactly: the seed can now be outside E (the j == seed branch)."""
    r, qs, ks = _maxima_subject(device, which, request)
    for name, mtw in E.under_estimates(r.mtw).items():
        wand = device.WandData(r.norm_lens, max_term_weight=mtw)
        for k in ks:
            want = ranked_want(ranked_or.ranked_or, r.lists, qs, r.norm_lens, r.num_docs, k)
            got = r.qi.ranked_or_maxscore_queries(r.fd, wand, qs, k=k)  # (DINT_OK, or DintError is raised)
            mods = [maxscore.maxscore(r.lists, q, r.norm_lens, mtw, r.num_docs, k) for q in qs]
            for i, m in enumerate(mods):
                maxscore.assert_degraded(got[0][i], got[1][i], got[2][i], m, int(want[0][i]))
            assert got[3] <= sum(m.all_blocks for m in mods)
            model = (np.array([m.count for m in mods], dtype=np.uint64), np.stack([m.scores for m in mods]), np.stack([m.ids for m in mods]))
            assert_ranked(got[:3], model, (which, name, k))
            assert got[3] == sum(m.blocks_read for m in mods), (which, name, k)
            if name == "zeros":
                assert not np.array_equal(got[2], want[2]), "these maxima do drop documents"
        wand.close()
    r.close()


def test_nan_and_negative_maxima_are_refused_at_creation(device, small_corpus):
    """A NaN among the maxima would hand std::sort a comparison that is no strict weak ordering (a query of 17 or more terms:
    undefined behaviour on the host); a negative one is no maximum of a non-negative weight. Both: DINT_ERR_ARG from
    dint_wand_data_create_with_max_weights, wherever in the array. -0.0, FLT_MAX and +inf are accepted."""
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    for bad in (np.nan, -np.nan, -1.0, -np.inf, -1e-45):
        for at in (0, len(r.mtw) // 2, len(r.mtw) - 1):
            mtw = r.mtw.copy()
            mtw[at] = bad
            with pytest.raises(device.DintError):
                device.WandData(r.norm_lens, max_term_weight=mtw)
    qs = [q for q in heavy_queries(ix.lens, 10)] + [list(range(20))]
    want = r.want(qs, 10)
    for good in (-0.0, E.FLT_MAX, np.inf):
        mtw = r.mtw.copy()
        mtw[:20:3] = good
        wand = device.WandData(r.norm_lens, max_term_weight=mtw)
        if good != 0:
            _assert_equal(r.qi.ranked_or_maxscore_queries(r.fd, wand, qs, k=10)[:3], want)
        wand.close()
    r.close()


# ---------------------------------------------------------------------------------------------------------------
# the hand-made edges (tests/maxscore_edges.py; tests/test_ranked_or_maxscore_cpu.py holds the model to the same specs)
# ---------------------------------------------------------------------------------------------------------------
class Hand(HandIndex):
    """A spec's lists through the project's encoder, with a wand handle that carries its exact maxima."""

    def __init__(self, device, kind, spec):
        super().__init__(device, kind, spec.lists, spec.freqs, spec.num_docs, spec.nl)
        self.spec = spec
        self.mwand = device.WandData(self.nl, max_term_weight=spec.mtw)

    def run_ms(self, qs, k):
        return self.qi.ranked_or_maxscore_queries(self.fd, self.mwand, qs, k=k)

    def check_spec(self):
        """Per k of the spec: its queries in one call and one per call: ranked_or's answer (model and device), the model's
        blocks read query by query, and the model as the spec knows it by construction (theta, the blocks counted by hand)."""
        spec, out = self.spec, {}
        for k in sorted({q.k for q in spec.queries}):
            queries = [q for q in spec.queries if q.k == k]
            qs = [q.terms for q in queries]
            want = ranked_want(ranked_or.ranked_or, self.lists, qs, self.nl, self.num_docs, k)
            mods = [spec.check_model(q) for q in queries]
            got = self.run_ms(qs, k)
            assert_ranked(got[:3], want, ("batch", k))
            assert_ranked(self.qi.ranked_or_queries(self.fd, self.wand, qs, k=k), want, ("ranked_or", k))
            assert got[3] == sum(m.blocks_read for m in mods), ("batch", k, [m.blocks_read for m in mods])
            for i, (q, m) in enumerate(zip(queries, mods)):
                one = self.run_ms([q.terms], k)
                assert_ranked(one[:3], tuple(a[i:i + 1] for a in want), q)
                assert one[3] == m.blocks_read, (q, one[3], m.blocks_read)
                out[id(q)] = one
        return [out[id(q)] for q in spec.queries]

    def close(self):
        super().close()
        self.mwand.close()


KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]


@pytest.mark.parametrize("i", range(len(E.LENGTH_CASES)), ids=lambda i: "k{}{}".format(E.LENGTH_CASES[i][0], "-equal" if E.LENGTH_CASES[i][1] else ""))
def test_list_lengths_on_k(device, i):
    """Lists of k - 1, k and k + 1 postings with two lists of 24 and 28 pages: the list of exactly k postings is the seed and
    theta its smallest addend; k - 1 postings are no seed; without a list of k postings theta is 0 and every block is read;
    of two lists of k postings the smaller term id is the seed."""
    k, equal = E.LENGTH_CASES[i]
    h = Hand(device, KINDS[i % 3], E.lengths_on_k(k, equal))
    h.check_spec()
    h.close()


@pytest.mark.parametrize("maker", [E.seed_ties, E.subnormal_theta], ids=lambda f: f.__name__)
def test_seed_ties_and_subnormal_thresholds(device, maker):
    h = Hand(device, host.RECTANGULAR, maker())
    h.check_spec()
    h.close()


def test_a_seed_whose_kth_addend_is_zero(device):
    spec = E.zero_theta()
    h = Hand(device, host.SINGLE_PACKED, spec)
    got = h.check_spec()
    assert int(got[3][0][0]) == 256 and got[3][1][0][255] == 0.0 and int(got[3][2][0][255]) == spec.zero_doc  # counted, last
    h.close()


@pytest.mark.parametrize("kind", KINDS)
def test_claim_geometry(device, kind):
    """Candidates on a block's last docID, below an N list's first and above its last docID, in its short last block, in
    blocks that do not hold them, 200 neighbours in one block, one block claimed from two E lists' pages, N lists of one
    block and of 80 pages with one and with all blocks claimed: the blocks read are those counted by hand."""
    spec = E.claim_geometry()
    h = Hand(device, kind, spec)
    h.check_spec()
    for pass_pages in (1, 1 << 20):  # every k = 2 query in one call, N lists shared between the queries of a pass or not
        with device.options(query_or_pass_pages=pass_pages):
            queries = [q for q in spec.queries if q.k == 2]
            got = h.run_ms([q.terms for q in queries] * 2, 2)
            assert got[3] == 2 * sum(q.blocks for q in queries)
    h.close()


def test_a_handle_reused_for_calls_of_different_sizes(device, small_corpus):
    """A large call, a small one, the large one again (and at another k) on one handle, each against a fresh handle: nothing
    of an earlier call's claim flags, ranks or workspace sizes shows in a later one."""
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    large = reference_queries(len(ix.lens))[:100] + heavy_queries(ix.lens, 40) + maxscore.mixed_queries(ix.lens, 40)
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    small = [[mid], maxscore.mixed_queries(ix.lens, 1, seed=3)[0]]
    calls = [(large, 10), (small, 10), (large, 10), (small, 1000), (large, 1000), (small, 1), (large[:7], 10), (large, 10)]
    r = Pruned(device, ix, kind)
    for qs, k in calls:
        fresh = Pruned(device, ix, kind)
        want = fresh.run_ms(qs, k)
        fresh.close()
        got = r.run_ms(qs, k)
        _assert_equal(got[:3], want[:3])
        assert got[3] == want[3]
    _assert_equal(r.run_ms(large, 10)[:3], r.want(large, 10))
    r.close()
