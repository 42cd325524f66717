"""Ranked boolean queries on the GPU through the C ABI (dint_ranked_bool_queries): counts, matches and docIDs equal to the
binary32 model (tests/ranked_bool.py), scores compared as bit patterns, blocks decoded equal to the model's for a query run
alone — over the three corpora and kinds, hand-made lists for the edges of blocks and lists, every launch form of the
ranked AND path, a seeded random case drawn as tests/query_fuzz_draws.py draws, and with the handle's other calls behind
it (claims released). tests/test_ranked_bool_cpu.py shows on the model that these inputs reorder, exclude and end early."""
import ctypes as C

import numpy as np
import pytest

import fuzz_streams as F
import ranked
import ranked_bool as RB
import score_documents as S
from dint_amd import host
from queries import heavy_queries, intersect_freqs, reference_queries
from query_fuzz_draws import draw_case
from test_gpu_query_fuzz import QUERY, HandIndex
from test_gpu_ranked_queries import Ranked
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]


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


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def assert_equal(got, want, what=None):
    """counts, matches, score bits, docIDs (the fifth of either: blocks decoded, compared by the caller)"""
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(bits(got[2]), bits(want[2])), what
    assert np.array_equal(got[3], want[3]), what


class Bool:
    """Anything with qi / fd / wand / lists, norm_lens and num_docs: the device call and the model over the same clauses."""

    def __init__(self, qi, fd, wand, lists, nl, num_docs):
        self.qi, self.fd, self.wand, self.lists, self.nl, self.num_docs = qi, fd, wand, lists, nl, num_docs

    @classmethod
    def of(cls, r):
        return cls(r.qi, r.fd, r.wand, r.lists, getattr(r, "norm_lens", getattr(r, "nl", None)), r.num_docs)

    def run(self, clauses, k):
        return self.qi.ranked_bool_queries(self.fd, self.wand, clauses[0], clauses[1], clauses[2], k=k)

    def want(self, clauses, k):
        return RB.model_batch(self.lists, clauses[0], clauses[1], clauses[2], self.nl, self.num_docs, k)

    def check(self, clauses, k, what=None):
        got, want = self.run(clauses, k), self.want(clauses, k)
        assert_equal(got, want, what)
        assert got[4] <= sum(want[4]), (what, got[4], sum(want[4]))
        if len(clauses[0]) == 1:
            assert got[4] == want[4][0], (what, got[4], want[4])
        return got, want


def part(clauses, idx):
    return tuple([c[i] for i in idx] for c in clauses)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_is_bit_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Ranked(device, ix, kind)
    b = Bool.of(r)
    clauses = RB.gpu_batch_clauses(ix.lens)
    for k in (10, 1, 1000):
        got, want = b.check(clauses, k, (corpus_name, k))
        if k == 10:
            assert int(want[1].sum()) > 500 and any(clauses[1]) and any(clauses[2])
    r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_without_optional_and_excluded_terms_it_is_ranked_and(device, small_corpus, kind):
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    qs = reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 60)
    for k in (10, 1000):
        want = r.run(qs, k)
        for should, exclude in ((None, None), ([[]] * len(qs), [[]] * len(qs))):
            got = r.qi.ranked_bool_queries(r.fd, r.wand, qs, should, exclude, k=k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[2]), bits(want[1])) and np.array_equal(got[3], want[2])
            assert np.array_equal(got[1], [intersect_freqs(ix.docids, ix.freqs, ix.bounds, q)[0] if len(q) else 0 for q in qs])
    one = r.qi.ranked_bool_queries(r.fd, r.wand, qs[-1:], k=10)
    assert one[4] == r.qi.and_queries_with_freqs(r.fd, qs[-1:])[2] > 0  # the required terms' claims are the freqs pass's
    r.close()


def _edge_index(device, kind):
    """0 A: two full blocks and a short one; 1 M: A's even places and a[255], a[511], and documents of its own — the matches
    of [A, M] lie at a[0], a[255], a[256], a[511], a[598]; 2: ends at the last match; 3, 5: end before the first match;
    4, 6: end after the last; 7: shorter than a block (interpolative); 8: ends among the matches, at a block's last place."""
    a = np.arange(10, 10 + 3 * 600, 3, dtype=np.uint32)
    m = np.unique(np.concatenate([a[::2], a[[255, 511]], np.arange(2000, 2300, dtype=np.uint32)])).astype(np.uint32)
    lists = [a, m, np.array([a[3], a[100], a[256], a[598]], dtype=np.uint32), np.array([0, 3, 5], dtype=np.uint32),
             np.array([a[255], a[300], 5000, 8000], dtype=np.uint32), np.array([1, 2, 4], dtype=np.uint32),
             np.arange(1500, 4000, 7, dtype=np.uint32), a[5:200:4].copy(), a[:256].copy()]
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 9, x.size).astype(np.uint32) for x in lists]
    num_docs = 9001
    nl = (rng.random(num_docs) * 2 + 0.1).astype(np.float32)
    return HandIndex(device, kind, lists, freqs, num_docs, nl), a


EDGE_MUST = [[0, 1], [0, 1], [0, 1], [0, 0, 1], [0, 1], [0, 1], [], [1], [0], [0, 1], []]
EDGE_SHOULD = [[], [7], [5, 6, 8], [8, 8], [1], [6], [6], [0, 7], [5], [4, 2], []]
EDGE_NOT = [[], [2, 4], [], [2, 2], [], [1], [2], [3, 4], [3], [6, 5], []]


@pytest.mark.parametrize("kind", KINDS)
def test_edges_of_lists_and_blocks(device, kind):
    h, a = _edge_index(device, kind)
    b = Bool.of(h)
    clauses = (EDGE_MUST, EDGE_SHOULD, EDGE_NOT)
    for k in (10, 1000):  # (1000: more than any query's matches)
        got, want = b.check(clauses, k, k)
        assert got[1].tolist() == want[1].tolist()
        for i in range(len(EDGE_MUST)):
            b.check(part(clauses, [i]), k, (k, i))  # alone: the blocks decoded are exact
    got, want = b.check(clauses, 1000)
    every = [set(got[3][i][:int(got[0][i])].tolist()) for i in range(len(EDGE_MUST))]
    lst = [set(x.tolist()) for x in h.lists.postings(2)[:1] + h.lists.postings(4)[:1]]
    assert every[0] == set(a[::2].tolist()) | {int(a[255]), int(a[511])}
    assert every[1] == every[0] - lst[0] - lst[1] and {int(a[255]), int(a[256]), int(a[598])}.isdisjoint(every[1]) and int(a[511]) in every[1]
    assert got[1].tolist() == [302, 297, 302, 299, 302, 0, 0, 600, 600, 295, 0]
    assert (got[3][6] == 0xFFFFFFFF).all() and (got[2][6] == 0).all()
    assert every[3] == every[0] - lst[0]
    # the same term required and optional: scored in both phases
    assert (got[2][4][:10] > got[2][0][:10]).all() and every[4] == every[0]
    # Blocks, for the queries alone. [A, M]: A's three blocks and the two of M's three that hold a match (its third: 2000 ..)
    assert want[4][0] == 3 + 2
    # lists 2 and 4 (a block each; a[255] is alive at list 4's step and every candidate lies before 8000), the required
    # terms', list 7 (one short block, matches below its last docID)
    assert want[4][1] == 1 + 1 + 5 + 1
    # list 5 ends before the first match: no claim; lists 6 and 8: the one block the matches up to its last docID fall in
    assert want[4][2] == 5 + 0 + 1 + 1
    # M excluded from [A, M]: its two blocks, then nothing is left to score
    assert want[4][5] == 2
    # [M] alone: list 3 ends before its first docID; list 4; M's three blocks; A's three (M's documents past A claim none); list 7
    assert want[4][7] == 0 + 1 + 3 + 3 + 1 and want[4][8] == 0 + 3 + 0
    # calls that launch nothing
    none = b.run(([], [], []), 10)
    assert none[0].size == 0 and none[2].shape == (0, 10) and none[4] == 0
    assert b.run(([[], []], [[6], []], [[2], []]), 10)[4] == 0
    h.close()


def test_blocks_decoded_exact_alone_bounded_in_a_batch_and_lazy(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    b = Bool.of(r)
    clauses = RB.split_clauses(heavy_queries(ix.lens, 40), ix.lens)
    got, want = b.check(clauses, 10)
    total = 0
    for i in range(0, len(clauses[0]), 3):
        one, _ = b.check(part(clauses, [i]), 10, i)
        total += one[4]
    assert total == sum(want[4][::3]) and 0 < got[4] <= sum(want[4])
    # tests/test_ranked_bool_cpu.py's floor: this heavy query claims a part of its terms' blocks
    (mu, sh, ex), claimed, every = RB.laziest_heavy_query(r.lists, ix.lens, r.norm_lens, r.num_docs)
    lazy = r.qi.ranked_bool_queries(r.fd, r.wand, [mu], [sh], [ex], k=10)
    assert lazy[4] == claimed and 0 < claimed < every
    r.close()


def test_claims_are_released_and_the_handle_is_left_as_found(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    b = Bool.of(r)
    clauses = part(RB.gpu_batch_clauses(ix.lens), range(0, 620, 5))
    n = len(clauses[0])
    first, want = b.check(clauses, 10)
    again = b.run(clauses, 10)
    assert_equal(again, first)
    assert again[4] == first[4]
    rev = b.run(part(clauses, range(n - 1, -1, -1)), 10)
    assert_equal(tuple(x[::-1] for x in rev[:4]), first)
    assert rev[4] == first[4]
    for i in range(0, n, 4):
        one = b.run(part(clauses, [i]), 10)
        assert_equal(one, tuple(x[i:i + 1] for x in first[:4]), i)
        assert one[4] == want[4][i]
    # the handle's other calls find their claim tables and workspaces as they need them
    qs = reference_queries(len(ix.lens))[::5] + heavy_queries(ix.lens, 12)
    want_and = r.want(qs, 10)
    got = r.run(qs, 10)
    assert np.array_equal(got[0], want_and[0]) and np.array_equal(bits(got[1]), bits(want_and[1])) and np.array_equal(got[2], want_and[2])
    fr = [intersect_freqs(ix.docids, ix.freqs, ix.bounds, q) for q in qs]
    counts, sums, _ = r.qi.and_queries_with_freqs(r.fd, qs)
    assert np.array_equal(counts, [f[0] for f in fr]) and np.array_equal(sums, [f[1] for f in fr])
    docs = [got[2][i][:int(got[0][i])] for i in range(len(qs))]
    scored = r.qi.score_documents(r.fd, r.wand, qs, docs)
    mods = S.model_batch(r.lists, qs, docs, r.norm_lens, r.num_docs)
    assert all(np.array_equal(bits(s), bits(m.scores)) for s, m in zip(scored[0], mods)) and scored[2] == sum(m.blocks_read for m in mods)
    assert_equal(b.run(clauses, 10), first)
    r.close()


@pytest.mark.parametrize("opts", [dict(), dict(query_fused_pages=0), dict(query_tail_pages=0, query_fused_pages=0),
                                  dict(query_lean_pages=0), dict(query_lean_pages=1 << 30, query_tail_pages=1 << 20)])
def test_every_launch_form(device, small_corpus, opts):
    """The fused, round-tail and batch-round forms of the ranked AND path, as tests/test_gpu_ranked_queries.py forces them: a
    batch, a heavy query alone and a query of a page or two of candidates alone (with the default options: the fused form)."""
    kind = host.RECTANGULAR
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    b = Bool.of(r)
    clauses = part(RB.gpu_batch_clauses(ix.lens), list(range(0, 500, 6)) + list(range(500, 520)))
    n = len(clauses[0])
    want = b.want(clauses, 10)
    full = [i for i in range(n) if clauses[1][i] and clauses[2][i] and want[1][i]]
    small = min(full, key=lambda i: min(int(ix.lens[t]) for t in clauses[0][i]))
    heavy = max(full, key=lambda i: min(int(ix.lens[t]) for t in clauses[0][i]))
    # (at most query_fused_pages = 2 candidate pages: fused, or a round tail with that form off; more than query_tail_pages = 4: batch rounds)
    assert min(int(ix.lens[t]) for t in clauses[0][small]) <= 2 * 256 and 4 * 256 < min(int(ix.lens[t]) for t in clauses[0][heavy])
    with device.options(**opts):
        got = b.run(clauses, 10)
        assert_equal(got, want, opts)
        for i in (heavy, small):
            one = b.run(part(clauses, [i]), 10)
            assert_equal(one, tuple(x[i:i + 1] for x in want[:4]), (opts, i))
            assert one[4] == want[4][i]
    r.close()


def test_refused_before_any_launch(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    n_lists = len(ix.lens)
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    run = lambda must, should, exclude, k=10, wand=r.wand: r.qi.ranked_bool_queries(r.fd, wand, must, should, exclude, k=k)  # noqa: E731
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            run([[mid]], None, None, k=bad_k)
    for clauses in (([[n_lists]], None, None), ([[mid]], [[n_lists]], None), ([[mid]], None, [[n_lists]]),
                    ([[]], [[n_lists]], None)):  # (checked even where the query selects nothing)
        with pytest.raises(device.DintError):
            run(*clauses)
    short = device.WandData(r.norm_lens[:int(ix.docids.max())])  # num_docs == the largest docID
    with pytest.raises(device.DintError):
        run([[mid]], None, None, wand=short)
    short.close()
    # decreasing offsets in each clause, through the bare entry
    lib = device._lib
    terms = np.array([mid, mid, mid], dtype=np.uint32)
    good, bad = np.array([0, 1, 2], dtype=np.uint64), np.array([0, 2, 1], dtype=np.uint64)
    counts, scores, blocks = np.zeros(2, dtype=np.uint64), np.zeros(20, dtype=np.float32), C.c_uint64(77)
    for which in range(3):
        offs = [bad if i == which else good for i in range(3)]
        assert lib.dint_ranked_bool_queries(r.qi._h, r.fd._h, r.wand._h, 10, terms.ctypes.data, offs[0].ctypes.data, terms.ctypes.data,
                                            offs[1].ctypes.data, terms.ctypes.data, offs[2].ctypes.data, 2, counts.ctypes.data, None,
                                            scores.ctypes.data, None, C.byref(blocks), None) == DINT_ERR_ARG
    # matches, docids and blocks_decoded may be null; a null must clause selects nothing
    assert lib.dint_ranked_bool_queries(r.qi._h, r.fd._h, r.wand._h, 10, terms.ctypes.data, good.ctypes.data, None, None, None, None, 2,
                                        counts.ctypes.data, None, scores.ctypes.data, None, None, None) == 0
    want = r.want([[mid], [mid]], 10)
    assert np.array_equal(counts, want[0]) and np.array_equal(bits(scores.reshape(2, 10)), bits(want[1]))
    assert lib.dint_ranked_bool_queries(r.qi._h, r.fd._h, r.wand._h, 10, None, None, terms.ctypes.data, good.ctypes.data, None, None, 2,
                                        counts.ctypes.data, None, scores.ctypes.data, None, C.byref(blocks), None) == 0
    assert (counts == 0).all() and (scores == 0).all() and blocks.value == 0
    r.close()


def _random_clauses(r, qs):
    """Every term of a drawn query goes to a clause of its own draw (repeats and shared terms included)."""
    must, should, exclude = [], [], []
    for q in qs:
        role = r.choice(3, len(q), p=[0.5, 0.3, 0.2])
        must.append([int(t) for t, c in zip(q, role) if c == 0])
        should.append([int(t) for t, c in zip(q, role) if c == 1])
        exclude.append([int(t) for t, c in zip(q, role) if c == 2])
    return must, should, exclude


@pytest.mark.parametrize("case", QUERY[:4], ids=lambda c: f"seed{c[0]}")
def test_seeded_random_case(device, case):
    """Lists, queries, norm_lens and k as the query fuzz draws them (four cases of about 60 queries each)."""
    Dd, Df, X = F.build_query_case(case)
    _, qs, nl, ks = draw_case(case[0], X)
    rng = np.random.default_rng(case[0] + 23)
    clauses = _random_clauses(rng, qs + qs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    qi = device.QueryIndex(dd, X.index, X.offsets)
    wand = device.WandData(nl)
    b = Bool(qi, fd, wand, ranked.BuilderLists(X.docids, X.freqs, X.bounds), nl, int(X.docids.max()) + 1)
    for k in ks:
        got, want = b.check(clauses, k, (case[0], k))
    assert int(want[1].sum()) > 0 and any(m and s and e for m, s, e in zip(*clauses))
    for i in range(0, len(clauses[0]), 9):
        b.check(part(clauses, [i]), ks[0], (case[0], i))
    qi.close()
    wand.close()
