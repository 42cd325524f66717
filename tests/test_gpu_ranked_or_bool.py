"""Union-driven ranked boolean queries on the GPU through the C ABI (dint_ranked_or_bool_queries): counts, matches and docIDs
equal to the binary32 model (tests/ranked_or_bool.py), scores compared as bit patterns, blocks decoded equal to the model's for
a query run alone — over the three corpora and kinds, hand-made lists for the edges of blocks and lists, passes of 1, 2 and 7
pages, a seeded random case drawn as tests/query_fuzz_draws.py draws, and with the handle's other calls before and behind it
(claims released). tests/test_ranked_or_bool_cpu.py shows on the model that these inputs filter, exclude and stay lazy."""
import ctypes as C

import numpy as np
import pytest

import fuzz_streams as F
import ranked
import ranked_bool as RB
import ranked_or_bool as ROB
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
_MODEL = {}  # corpus name -> (clauses, the batch evaluated): the same for every kind


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


class OrBool:
    """Anything with qi / fd / wand / lists, norm_lens and num_docs: the device call and the model over the same clauses
    (should, exclude, min_should_match)."""

    def __init__(self, qi, fd, wand, lists, nl, num_docs):
        self.qi, self.fd, self.wand, self.lists, self.nl, self.num_docs = qi, fd, wand, lists, nl, num_docs

    @classmethod
    def of(cls, r):
        return cls(r.qi, r.fd, r.wand, r.lists, getattr(r, "norm_lens", getattr(r, "nl", None)), r.num_docs)

    def run(self, clauses, k):
        return self.qi.ranked_or_bool_queries(self.fd, self.wand, clauses[0], clauses[1], clauses[2], k=k)

    def evaluate(self, clauses):
        return ROB.evaluate_batch(self.lists, clauses[0], clauses[1], clauses[2], self.nl, self.num_docs)

    def check(self, clauses, k, what=None, evs=None):
        got = self.run(clauses, k)
        want = ROB.top_batch(evs if evs is not None else self.evaluate(clauses), k)
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
    b = OrBool.of(r)
    if corpus_name not in _MODEL:
        clauses = ROB.gpu_batch_clauses(ix.lens)
        _MODEL[corpus_name] = (clauses, b.evaluate(clauses))
    clauses, evs = _MODEL[corpus_name]
    for k in (10, 1, 1000):
        got, want = b.check(clauses, k, (corpus_name, k), evs)
        if k == 10:
            assert int(want[1].sum()) > 500 and any(clauses[1]) and max(clauses[2]) >= 2
    # alone, the blocks decoded are exact: queries of every kind of the derivation, and the heavy ones
    n = len(clauses[0])
    for i in list(range(0, 40, 3)) + list(range(n - 12, n)):
        b.check(part(clauses, [i]), 10, (corpus_name, i), evs[i:i + 1])
    r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_without_a_minimum_and_exclusions_it_is_ranked_or(device, small_corpus, kind):
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    qs = reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 60)
    for k in (10, 1000):
        want = r.qi.ranked_or_queries(r.fd, r.wand, qs, k=k)
        for exclude, mins in ((None, None), ([[]] * len(qs), [0] * len(qs)), (None, [1] * len(qs))):
            got = r.qi.ranked_or_bool_queries(r.fd, r.wand, qs, exclude, mins, k=k)
            assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[2]), bits(want[1])) and np.array_equal(got[3], want[2])
            assert np.array_equal(np.minimum(got[1], k), want[0])
    r.close()


def test_every_returned_score_is_score_documents(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    clauses = part(ROB.gpu_batch_clauses(ix.lens), range(0, 620, 5))
    got = OrBool.of(r).run(clauses, 10)
    docs = [got[3][i][:int(got[0][i])] for i in range(len(clauses[0]))]
    assert sum(d.size for d in docs) > 300
    scored = r.qi.score_documents(r.fd, r.wand, clauses[0], docs)[0]
    for i, s in enumerate(scored):
        assert np.array_equal(bits(s), bits(got[2][i][:docs[i].size])), i
    r.close()


def _edge_index(device, kind):
    """0 A: two full blocks and a short one (600 postings); 1 B: shorter than a block (interpolative), partly in A; 2 C: A's
    first 256 — a full block that ends at a block's last place; 3: ends before the first candidate; 4: ends after the last;
    5: A's second block — it ends exactly at a[511], a candidate and a block's last docID; 6 D: a full block and a short one
    of documents of its own; 7: empty — the index builder cannot write an empty list, so the handle is made again through the
    bare entry over the same index and block table with one list more, which no block names."""
    a = np.arange(10, 10 + 3 * 600, 3, dtype=np.uint32)
    lists = [a, np.unique(np.concatenate([a[5:200:4], np.arange(11, 400, 30, dtype=np.uint32)])).astype(np.uint32), a[:256].copy(),
             np.array([0, 3, 5], dtype=np.uint32), np.array([a[255], a[300], 5000, 8000], dtype=np.uint32), a[256:512].copy(),
             np.arange(1500, 4000, 7, dtype=np.uint32)]
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 9, x.size).astype(np.uint32) for x in lists]
    num_docs = 9001
    nl = (rng.random(num_docs) * 2 + 0.1).astype(np.float32)
    h = HandIndex(device, kind, lists, freqs, num_docs, nl)
    qi, wider = h.qi, C.c_void_p()
    assert device._lib.dint_query_index_create(qi.docs_dict._h, qi._index_dev.data_ptr(), qi._index_dev.numel(), qi.blocks.ctypes.data,
                                               len(qi.blocks), qi.n_lists + 1, C.byref(wider)) == 0
    qi.close()
    qi._h, qi.n_lists = wider, qi.n_lists + 1
    h.lists = ranked.BuilderLists(h.docids, h.freqs, np.append(h.bounds, h.bounds[-1]))
    assert h.lists.postings(7)[0].size == 0
    return h, a


#              0    1       2       3          4       5    6       7                8   9    10         11   12      13   14      15
EDGE_SHOULD = [[0], [0, 1], [0, 1], [0, 1, 2], [0, 1], [0], [0, 2], [0, 0, 1, 1, 1], [], [], [6, 1, 2], [2], [0, 6], [7], [0, 7], [7, 0]]
EDGE_NOT = [[], [], [], [3], [4], [5], [2], [4, 4], [], [4], [0], [0], [5, 3, 6], [], [7], [3]]
EDGE_MIN = [1, 2, 3, 1, 1, 1, 1, 2, 1, 1, 2, 1, 0, 1, 1, 2]


@pytest.mark.parametrize("kind", KINDS)
def test_edges_of_lists_and_blocks(device, kind):
    h, a = _edge_index(device, kind)
    b = OrBool.of(h)
    clauses = (EDGE_SHOULD, EDGE_NOT, EDGE_MIN)
    evs = b.evaluate(clauses)
    n = len(EDGE_SHOULD)
    for k in (10, 1000):  # (1000: more than any query's matches)
        b.check(clauses, k, k, evs)
        for i in range(n):
            b.check(part(clauses, [i]), k, (k, i), evs[i:i + 1])  # alone: the blocks decoded are exact
    got, want = b.check(clauses, 1000, None, evs)
    every = [set(got[3][i][:int(got[0][i])].tolist()) for i in range(n)]
    A, B, Cl, X5, D = (set(h.lists.postings(t)[0].tolist()) for t in (0, 1, 2, 5, 6))
    own = len(B - A)
    assert own > 0 and len(A & B) == 49 and Cl < A and X5 < A and 0 < len(D & A) < len(D)
    two_of = ((B & Cl) | (B & D) | (Cl & D)) - A  # query 10: in two of D, B and C, and not in A
    assert got[1].tolist() == [600, 49, 0, 600 + own, 600 + own - 2, 600 - 256, 600 - 256, 49, 0, 0, len(two_of), 0, len(A - X5 - D),
                                0, 600, 0]
    assert every[1] == A & B and every[6] == A - Cl and every[5] == A - X5 and every[10] == two_of
    assert {int(a[255]), int(a[300])}.isdisjoint(every[4]) and int(a[511]) not in every[5] and int(a[512]) in every[5]
    for i in (2, 8, 9, 11, 13, 15):
        assert (got[3][i] == 0xFFFFFFFF).all() and (got[2][i] == 0).all()
    # Blocks, for the queries alone. A: three; m = 2 over [A, B] decodes both lists whole; m above the terms: nothing
    assert [want[4][i] for i in (0, 1, 2)] == [3, 4, 0]
    # list 3 ends before the first candidate: no claim; list 4's one block: every candidate lies before 8000
    assert want[4][3] == 3 + 1 + 1 + 0 and want[4][4] == 3 + 1 + 1
    # list 5 ends at a[511]: the candidates up to it claim its one block, the ones past it nothing; C in both clauses: claimed once
    assert want[4][5] == 3 + 1 and want[4][6] == 3 + 1 + 1
    # repeats in `not` are one step; an empty query and a query of excluded terms only launch nothing
    assert want[4][7] == 3 + 1 + 1 and want[4][8] == want[4][9] == 0
    # A excluded from C: C's block, then the one block of A its documents fall in; nothing is left
    assert want[4][11] == 1 + 1
    # [A, D] less lists 3, 5 and D itself: D's documents past A claim no block of list 5, D's two blocks are claimed by D's own
    assert want[4][12] == 3 + 2 + 0 + 1 + 2 and every[12] == A - X5 - D
    # the empty list: alone nothing to decode; excluded it claims nothing; asked for beside A, A is decoded and nothing matches
    assert [want[4][i] for i in (13, 14, 15)] == [0, 3, 3] and every[14] == A
    # calls that launch nothing
    none = b.run(([], [], []), 10)
    assert none[0].size == 0 and none[2].shape == (0, 10) and none[4] == 0
    assert b.run(([[], []], [[6], []], [2, 0]), 10)[4] == 0
    h.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_passes(device, small_corpus, pass_pages):
    """query_or_pass_pages cuts the call into many passes (a query larger than the bound alone in a pass sized to it): the
    answers and the one-query block counts stay what they are."""
    kind = host.RECTANGULAR
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    b = OrBool.of(r)
    clauses = part(ROB.gpu_batch_clauses(ix.lens), list(range(0, 500, 6)) + list(range(500, 520)))
    evs = b.evaluate(clauses)
    whole = b.run(clauses, 10)
    with device.options(query_or_pass_pages=pass_pages):
        got, want = b.check(clauses, 10, pass_pages, evs)
        assert_equal(got, whole)
        heavy = max(range(len(evs)), key=lambda i: evs[i].blocks if clauses[1][i] and evs[i].docs.size else 0)
        assert evs[heavy].eager > 7 and evs[heavy].lazy
        b.check(part(clauses, [heavy]), 10, (pass_pages, heavy), evs[heavy:heavy + 1])
    r.close()


def test_claims_are_released_and_the_handle_is_left_as_found(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    b = OrBool.of(r)
    qs = reference_queries(len(ix.lens))[::5] + heavy_queries(ix.lens, 12)
    bool_clauses = RB.split_clauses(qs, ix.lens)

    def others():
        ra = r.run(qs, 10)
        fr = r.qi.and_queries_with_freqs(r.fd, qs)
        rb = r.qi.ranked_bool_queries(r.fd, r.wand, *bool_clauses, k=10)
        ro = r.qi.ranked_or_queries(r.fd, r.wand, qs, k=10)
        docs = [ro[2][i][:int(ro[0][i])] for i in range(len(qs))]
        sd = r.qi.score_documents(r.fd, r.wand, qs, docs)
        return ra, fr, rb, ro, sd

    def same(x, y):
        for g, w in zip(x, y):
            for u, v in zip(g, w):
                if isinstance(u, list):
                    assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(u, v))
                elif isinstance(u, np.ndarray):
                    assert np.array_equal(u.view(np.uint32) if u.dtype == np.float32 else u, v.view(np.uint32) if v.dtype == np.float32 else v)
                else:
                    assert u == v

    before = others()
    # ... and they are right: the models of the four calls
    want_and = r.want(qs, 10)
    assert np.array_equal(before[0][0], want_and[0]) and np.array_equal(bits(before[0][1]), bits(want_and[1]))
    fr = [intersect_freqs(ix.docids, ix.freqs, ix.bounds, q) for q in qs]
    assert np.array_equal(before[1][0], [f[0] for f in fr]) and np.array_equal(before[1][1], [f[1] for f in fr])
    want_bool = RB.model_batch(r.lists, *bool_clauses, r.norm_lens, r.num_docs, 10)
    assert np.array_equal(before[2][1], want_bool[1]) and np.array_equal(bits(before[2][2]), bits(want_bool[2]))
    mods = S.model_batch(r.lists, qs, [before[3][2][i][:int(before[3][0][i])] for i in range(len(qs))], r.norm_lens, r.num_docs)
    assert all(np.array_equal(bits(s), bits(m.scores)) for s, m in zip(before[4][0], mods))

    clauses = part(ROB.gpu_batch_clauses(ix.lens), range(0, 620, 5))
    n = len(clauses[0])
    evs = b.evaluate(clauses)
    first, want = b.check(clauses, 10, None, evs)
    assert first[4] > sum(e.eager for e in evs) and any(e.blocks > e.eager for e in evs)  # (the eager part is exact in a batch too)
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
    same(others(), before)
    assert_equal(b.run(clauses, 10), first)
    r.close()


def test_refused_before_any_launch(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    n_lists = len(ix.lens)
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    run = lambda should, exclude, mins=None, k=10, wand=r.wand: r.qi.ranked_or_bool_queries(r.fd, wand, should, exclude, mins, k=k)  # noqa: E731
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            run([[mid]], None, k=bad_k)
    for clauses in (([[n_lists]], None), ([[mid]], [[n_lists]]), ([[]], [[n_lists]]), ([[mid]], [[n_lists]], [5])):
        with pytest.raises(device.DintError):  # (checked even where the query selects nothing)
            run(*clauses)
    short = device.WandData(r.norm_lens[:int(ix.docids.max())])  # num_docs == the largest docID
    with pytest.raises(device.DintError):
        run([[mid]], None, wand=short)
    short.close()
    other = device.Dictionary(host.RECTANGULAR, get_index(small_corpus, host.RECTANGULAR).freqs_dict)  # a freqs dictionary of another kind
    with pytest.raises(device.DintError):
        r.qi.ranked_or_bool_queries(other, r.wand, [[mid]], k=10)
    # through the bare entry: decreasing offsets in either clause, null counts / scores / offsets, terms missing — and the
    # outputs are left as they were
    lib = device._lib
    terms = np.array([mid, mid, mid], dtype=np.uint32)
    good, bad = np.array([0, 1, 2], dtype=np.uint64), np.array([0, 2, 1], dtype=np.uint64)
    counts, matches = np.full(2, 7, dtype=np.uint64), np.full(2, 8, dtype=np.uint64)
    scores, docids, blocks = np.full(20, 3.5, dtype=np.float32), np.full(20, 9, dtype=np.uint32), C.c_uint64(77)
    ptr = lambda x: x.ctypes.data if x is not None else None  # noqa: E731

    def bare(s_terms, s_offs, x_terms, x_offs, k=10, counts_=counts, scores_=scores, qi=r.qi._h, fd=r.fd._h, wand=r.wand._h):
        return lib.dint_ranked_or_bool_queries(qi, fd, wand, k, ptr(s_terms), ptr(s_offs), ptr(x_terms), ptr(x_offs), None, 2, ptr(counts_),
                                               matches.ctypes.data, ptr(scores_), docids.ctypes.data, C.byref(blocks), None)

    huge = np.array([mid, n_lists, mid], dtype=np.uint32)
    for args in ((terms, bad, terms, good), (terms, good, terms, bad), (terms, None, None, None), (None, good, None, None),
                 (terms, good, None, good), (huge, good, None, None), (terms, good, huge, good)):
        assert bare(*args) == DINT_ERR_ARG, args
    assert bare(terms, good, None, None, counts_=None) == DINT_ERR_ARG and bare(terms, good, None, None, scores_=None) == DINT_ERR_ARG
    assert bare(terms, good, None, None, k=0) == DINT_ERR_ARG and bare(terms, good, None, None, k=1025) == DINT_ERR_ARG
    assert bare(terms, good, None, None, qi=None) == bare(terms, good, None, None, fd=None) == bare(terms, good, None, None, wand=None) == DINT_ERR_ARG
    assert (counts == 7).all() and (matches == 8).all() and (scores == 3.5).all() and (docids == 9).all() and blocks.value == 77
    # matches, docids, blocks_decoded, min_should_match and the `not` pair may be null
    assert lib.dint_ranked_or_bool_queries(r.qi._h, r.fd._h, r.wand._h, 10, terms.ctypes.data, good.ctypes.data, None, None, None, 2,
                                           counts.ctypes.data, None, scores.ctypes.data, None, None, None) == 0
    want = ROB.model_batch(r.lists, [[mid], [mid]], None, None, r.norm_lens, r.num_docs, 10)
    assert np.array_equal(counts, want[0]) and np.array_equal(bits(scores.reshape(2, 10)), bits(want[2]))
    r.close()


def _random_clauses(r, qs):
    """Every term of a drawn query goes to a clause of its own draw (repeats and shared terms included); m from 0 to one above
    the optional terms."""
    should, exclude, mins = [], [], []
    for q in qs:
        role = r.choice(2, len(q), p=[0.75, 0.25])
        should.append([int(t) for t, c in zip(q, role) if c == 0])
        exclude.append([int(t) for t, c in zip(q, role) if c == 1])
        mins.append(int(r.integers(0, min(4, len(set(should[-1])) + 2))))
    return should, exclude, mins


def test_seeded_random_case(device):
    """Lists, queries, norm_lens, the pass size and k as the query fuzz draws them (one case, about 120 queries)."""
    case = QUERY[0]
    Dd, Df, X = F.build_query_case(case)
    setting, qs, nl, ks = draw_case(case[0], X)
    rng = np.random.default_rng(case[0] + 29)
    clauses = _random_clauses(rng, qs + qs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    qi = device.QueryIndex(dd, X.index, X.offsets)
    wand = device.WandData(nl)
    b = OrBool(qi, fd, wand, ranked.BuilderLists(X.docids, X.freqs, X.bounds), nl, int(X.docids.max()) + 1)
    evs = b.evaluate(clauses)
    with device.options(query_or_pass_pages=setting["query_or_pass_pages"]):
        for k in ks:
            got, want = b.check(clauses, k, (case[0], k), evs)
        assert int(want[1].sum()) > 0 and any(s and e and m >= 2 for s, e, m in zip(*clauses))
        for i in range(0, len(clauses[0]), 9):
            b.check(part(clauses, [i]), ks[0], (case[0], i), evs[i:i + 1])
    qi.close()
    wand.close()
