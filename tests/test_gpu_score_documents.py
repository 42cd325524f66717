"""Scores of caller-given documents on the GPU through the C ABI (dint_score_documents): scores bit-equal to the model
(tests/score_documents.py: ranked_or's sums over next_geq + freq), the freqs matrices and the blocks read equal to the
model's — over the three corpora and kinds, the log / heavy / mixed query sets, the norm_lens classes of the ranked tests,
document sets from one document to the whole union, misses, repeats, the edges of lists and blocks, docIDs past the index
and near 2^32; against dint_ranked_or_queries' and dint_ranked_and_queries' own answers; and under every call form: passes
of 1, 2 and 7 pages, one query per call, the batch reversed and doubled, two host threads, a handle shared with the AND,
OR and pruned calls."""
import ctypes as C
import threading

import numpy as np
import pytest

import maxscore
import ranked
import score_documents as S
from dint_amd import host
from queries import heavy_queries, intersect, reference_queries
from query_fuzz_draws import NORM_LENS, draw_norm_lens
from test_gpu_query_fuzz import HandIndex
from test_gpu_query_high_docids import TOP, HighIndex, _high_lists
from test_gpu_ranked_or_maxscore import Pruned
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


def assert_model(got, mods, what=None):
    scores, freqs, blocks = got
    assert len(scores) == len(mods)
    for i, m in enumerate(mods):
        assert np.array_equal(bits(scores[i]), bits(m.scores)), (what, i)
        if freqs is not None:
            assert freqs[i].shape == m.freqs.shape and np.array_equal(freqs[i], m.freqs), (what, i)
    assert blocks == sum(m.blocks_read for m in mods), (what, blocks)


def check(qi, fd, wand, lists, nl, num_docs, qs, docs, what=None):
    """device == model for scores, freqs matrices and blocks read; the call without freqs gives the same scores and blocks."""
    mods = S.model_batch(lists, qs, docs, nl, num_docs)
    got = qi.score_documents(fd, wand, qs, docs, with_freqs=True)
    assert_model(got, mods, what)
    plain = qi.score_documents(fd, wand, qs, docs)
    assert plain[1] is None
    assert_model(plain, mods, what)
    return got, mods


def check_r(r, qs, docs, what=None):
    return check(r.qi, r.fd, r.wand, r.lists, r.norm_lens, r.num_docs, qs, docs, what)


def document_sets(r, rng, qs):
    """Per query, in turn: the whole union (of a small one), 1, 64 and 5 000 random documents of the union, random docIDs
    below num_docs (mostly misses), unsorted documents with repeats, nothing."""
    out = []
    for i, q in enumerate(qs):
        u = S.union_of(r.lists, q)
        which = i % 7
        if which == 0 and u.size <= 20000:
            d = u
        elif which in (0, 1):
            d = S.draw_from_union(rng, r.lists, q, 1)
        elif which == 2:
            d = S.draw_from_union(rng, r.lists, q, 64)
        elif which == 3:
            d = S.draw_from_union(rng, r.lists, q, 5000)
        elif which == 4:
            d = rng.integers(0, r.num_docs, 300).astype(np.uint32)
        elif which == 5:
            d = np.concatenate([S.draw_from_union(rng, r.lists, q, 200), rng.integers(0, r.num_docs, 50).astype(np.uint32)])
            d = rng.permutation(np.concatenate([d, d[:100], d[:10]])).astype(np.uint32)
        else:
            d = np.zeros(0, np.uint32)
        out.append(np.asarray(d, dtype=np.uint32))
    return out


def query_sets(ix):
    return reference_queries(len(ix.lens))[::4] + heavy_queries(ix.lens, 30) + maxscore.mixed_queries(ix.lens, 30)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Pruned(device, ix, kind)
    qs = query_sets(ix)
    rng = np.random.default_rng(100 + kind)
    docs = document_sets(r, rng, qs)
    got, mods = check_r(r, qs, docs)
    assert sum(int(m.held.any(axis=1).sum()) for m in mods) > 1000, "the sets hold documents of the lists"
    assert sum(int((~m.held.any(axis=1)).sum()) for m in mods) > 100, "and documents of none"
    assert got[2] <= sum(m.all_blocks for m in mods)
    r.close()


@pytest.mark.parametrize("cls", NORM_LENS)
def test_the_norm_lens_classes(device, small_corpus, cls):
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    rng = np.random.default_rng(7 + NORM_LENS.index(cls))
    nl = draw_norm_lens(rng, int(ix.docids.max()) + 1, cls)
    r = Pruned(device, ix, kind, norm_lens=nl)
    qs = query_sets(ix)[::2]
    check_r(r, qs, document_sets(r, rng, qs), cls)
    r.close()


def test_few_documents_read_few_blocks(device, small_corpus):
    """tests/test_score_documents_cpu.py's floor, on the device: 64 documents a heavy query read what the model reads, under six
    tenths of the queries' blocks — and dint_or_queries_freqs reads them all."""
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    rng = np.random.default_rng(13)
    qs = heavy_queries(ix.lens, 40)
    docs = [S.draw_from_union(rng, r.lists, q, 64) for q in qs]
    got, mods = check_r(r, qs, docs)
    all_blocks = sum(m.all_blocks for m in mods)
    assert r.qi.or_queries_with_freqs(r.fd, qs)[2] == all_blocks
    assert 0 < got[2] * 10 < all_blocks * 6
    r.close()


def _edge_index(device, kind):
    a = np.arange(10, 10 + 3 * 600, 3, dtype=np.uint32)   # 2 full blocks and a short one of 88
    b = np.arange(5000, 5300, dtype=np.uint32)            # a full block and a short one of 44
    c = np.array([0, 4000, 9000], dtype=np.uint32)
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 9, x.size).astype(np.uint32) for x in (a, b, c)]
    num_docs = 9001
    nl = (rng.random(num_docs) * 2 + 0.1).astype(np.float32)
    return HandIndex(device, kind, [a, b, c], freqs, num_docs, nl), a, b, c


@pytest.mark.parametrize("kind", KINDS)
def test_edges_of_lists_and_blocks(device, kind):
    h, a, b, c = _edge_index(device, kind)
    edge = np.array([0, a[0] - 1, a[0], a[0] + 1, a[255], a[255] + 1, a[256], a[511], a[511] + 1, a[550], a[599], a[599] + 1,
                     b[0], b[255], b[256], b[299], b[299] + 1, 4000, 9000, 9001, 20000, 0xFFFFFFFE, 0xFFFFFFFF], dtype=np.uint32)
    run = lambda qs, docs: check(h.qi, h.fd, h.wand, h.lists, h.nl, h.num_docs, qs, docs)
    none = np.zeros(0, np.uint32)
    # every edge under every query; empty queries and empty document sets in the middle of the batch
    qs = [[0], [1], [], [0, 1], [2], [0, 1, 2], [1], [2, 2, 0], []]
    docs = [edge, edge, edge, edge[::-1], edge, edge, none, np.concatenate([edge, edge]), none]
    got, mods = run(qs, docs)
    assert [m.blocks_read for m in mods] == [3, 2, 0, 5, 1, 6, 0, 4, 0]
    assert (got[0][2] == 0).all() and got[1][2].shape == (edge.size, 0)
    # past the index, and past norm_lens: in no list
    assert all((bits(s)[np.isin(d, [9001, 20000, 0xFFFFFFFE, 0xFFFFFFFF])] == 0).all() for s, d in zip(got[0], docs) if d.size)
    # one document a call: the block it falls in, and only where there is one
    for d, blocks in ((a[255], 1), (a[255] + 1, 1), (a[599], 1), (a[599] + 1, 0), (0, 1), (0xFFFFFFFF, 0)):
        one, _ = run([[0]], [np.array([d], dtype=np.uint32)])
        assert one[2] == blocks, (d, one[2])
        assert (one[0][0][0] != 0) == bool(np.isin(d, a)), d
    # calls that launch nothing
    assert run([], [])[0][0] == []
    assert run([[0, 1], []], [none, none])[0][2] == 0
    h.close()


@pytest.mark.parametrize("k", [10, 1000])
def test_the_answers_of_the_ranked_calls(device, small_corpus, k):
    """Over the ids dint_ranked_or_queries returned: that call's scores, bit for bit. Over dint_ranked_and_queries' ids: the
    model (ranked_and sums in list-length order, so its own scores may differ in the last bits)."""
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = query_sets(ix)
    counts, scores, ids = r.run(qs, k)
    docs = [ids[i][:int(counts[i])] for i in range(len(qs))]
    assert sum(d.size for d in docs) > 10 * len(qs) // 2
    got, _ = check_r(r, qs, docs, ("ranked_or", k))
    for i in range(len(qs)):
        assert np.array_equal(bits(got[0][i]), bits(scores[i][:int(counts[i])])), i
    pruned = r.run_ms(qs, k)
    for i in range(len(qs)):
        assert np.array_equal(bits(got[0][i]), bits(pruned[1][i][:int(pruned[0][i])])), i
    counts, _, ids = r.run_and(qs, k)
    docs = [ids[i][:int(counts[i])] for i in range(len(qs))]
    got, mods = check_r(r, qs, docs, ("ranked_and", k))
    assert all(m.held.all() for m in mods if m.held.size), "a document of the intersection is in every list"
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = query_sets(ix)[::2] + [[], [0]]
    rng = np.random.default_rng(3)
    docs = document_sets(r, rng, qs)
    one = r.qi.score_documents(r.fd, r.wand, qs, docs, with_freqs=True)
    device.set_option("query_or_pass_pages", pass_pages)
    got, _ = check_r(r, qs, docs, pass_pages)
    assert got[2] == one[2]
    for i in range(len(qs)):
        assert np.array_equal(bits(got[0][i]), bits(one[0][i])) and np.array_equal(got[1][i], one[1][i])
    r.close()


def test_batch_one_at_a_time_reversed_and_twice(device, small_corpus):
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = query_sets(ix)[::2]
    rng = np.random.default_rng(4)
    docs = document_sets(r, rng, qs)
    batch, mods = check_r(r, qs, docs)
    total = 0
    for i, (q, d) in enumerate(zip(qs, docs)):
        one = r.qi.score_documents(r.fd, r.wand, [q], [d], with_freqs=True)
        assert np.array_equal(bits(one[0][0]), bits(batch[0][i])) and np.array_equal(one[1][0], batch[1][i])
        assert one[2] == mods[i].blocks_read
        total += one[2]
    assert total == batch[2]
    rev = r.qi.score_documents(r.fd, r.wand, qs[::-1], docs[::-1], with_freqs=True)
    assert_model(rev, mods[::-1], "reversed")
    for pass_pages in (3, 1 << 20):  # (two queries of a pass with the same terms claim apart)
        with device.options(query_or_pass_pages=pass_pages):
            twice = r.qi.score_documents(r.fd, r.wand, [q for q in qs for _ in range(2)], [d for d in docs for _ in range(2)], with_freqs=True)
            assert_model(twice, [m for m in mods for _ in range(2)], "twice")
            assert twice[2] == 2 * batch[2]
    r.close()


def test_one_handle_under_two_threads(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    qs = query_sets(ix)[::2]
    docs = document_sets(r, np.random.default_rng(6), qs)
    mods = S.model_batch(r.lists, qs, docs, r.norm_lens, r.num_docs)
    want_or = r.want(qs, 10)
    want_and = np.array([intersect(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            for _ in range(3):
                if which == 0:
                    assert_model(r.qi.score_documents(r.fd, r.wand, qs, docs, with_freqs=True), mods, "thread 0")
                    assert np.array_equal(r.qi.and_queries(qs), want_and)
                else:
                    got = r.run(qs, 10)
                    assert np.array_equal(bits(got[1]), bits(want_or[1])) and np.array_equal(got[2], want_or[2])
                    assert_model(r.qi.score_documents(r.fd, r.wand, qs[::-1], docs[::-1]), mods[::-1], "thread 1")
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert_model(r.qi.score_documents(r.fd, r.wand, qs, docs, with_freqs=True), mods, "plain")
    r.close()


def test_a_handle_shared_with_the_other_calls(device, small_corpus):
    """Between AND, AND with freqs, OR, ranked and pruned calls, at several sizes, and against a fresh handle: nothing of a
    call's claim flags, ranks or workspaces shows in the next; and the AND calls find their claim tables clean afterwards."""
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    large = query_sets(ix)
    small = large[-3:]
    rng = np.random.default_rng(8)
    sets = [(qs, document_sets(r, rng, qs)) for qs in (large, small, large[:7], large[::-1])]
    want_and = np.array([intersect(ix.docids, ix.bounds, q) for q in large], dtype=np.uint64)
    freqs_and = r.qi.and_queries_with_freqs(r.fd, large)
    want_or = r.qi.or_queries(large)
    pruned = r.run_ms(large, 10)
    for qs, docs in sets + sets[::-1]:
        check_r(r, qs, docs)
        assert np.array_equal(r.qi.and_queries(large), want_and)
        check_r(r, qs, docs)
        got = r.qi.and_queries_with_freqs(r.fd, large)
        assert np.array_equal(got[0], freqs_and[0]) and np.array_equal(got[1], freqs_and[1]) and got[2] == freqs_and[2]
        assert np.array_equal(r.qi.or_queries(large), want_or)
        check_r(r, qs[:5], docs[:5])
        again = r.run_ms(large, 10)
        assert np.array_equal(bits(again[1]), bits(pruned[1])) and np.array_equal(again[2], pruned[2]) and again[3] == pruned[3]
        with device.options(query_batch_fused=0, query_fused_pages=0, query_tail_pages=0):
            assert np.array_equal(r.qi.and_queries(large), want_and)
    fresh = Pruned(device, ix, kind)
    a = fresh.qi.score_documents(fresh.fd, fresh.wand, *sets[0], with_freqs=True)
    b = r.qi.score_documents(r.fd, r.wand, *sets[0], with_freqs=True)
    assert a[2] == b[2] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[0], b[0]))
    fresh.close()
    r.close()


def test_refused_before_any_launch(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Pruned(device, ix, kind)
    mid = int(np.flatnonzero((ix.lens >= 20) & (ix.lens < 1000))[0])
    d = [np.arange(5, dtype=np.uint32)]
    with pytest.raises(device.DintError):  # a term that is no list
        r.qi.score_documents(r.fd, r.wand, [[len(ix.lens)]], d)
    top = int(ix.docids.max())
    short = device.WandData(r.norm_lens[:top])  # num_docs == the largest docID
    with pytest.raises(device.DintError):
        r.qi.score_documents(r.fd, short, [[mid]], d)
    short.close()
    other = device.Dictionary(host.MULTI_PACKED, get_index(small_corpus, host.MULTI_PACKED).freqs_dict)  # another kind
    with pytest.raises(device.DintError):
        r.qi.score_documents(other, r.wand, [[mid]], d)
    # a handle with maxima is as good; freqs and blocks_read may be null
    lib = device._lib
    terms, offs = np.array([mid], dtype=np.uint32), np.array([0, 1], dtype=np.uint64)
    docs = np.ascontiguousarray(r.lists.postings(mid)[0][:5], dtype=np.uint32)
    doc_offs = np.array([0, 5], dtype=np.uint64)
    scores = np.zeros(5, dtype=np.float32)
    assert lib.dint_score_documents(r.qi._h, r.fd._h, r.mwand._h, terms.ctypes.data, offs.ctypes.data, 1, docs.ctypes.data,
                                    doc_offs.ctypes.data, scores.ctypes.data, None, None, None) == 0
    want = S.score_documents(r.lists, [mid], docs, r.norm_lens, r.num_docs)
    assert np.array_equal(bits(scores), bits(want.scores)) and (scores > 0).all()
    # offsets that do not begin at 0: scores lie like docids
    docs2 = np.concatenate([np.full(3, 77, np.uint32), docs])
    scores2 = np.full(8, -1.0, dtype=np.float32)
    doc_offs2 = np.array([3, 8], dtype=np.uint64)
    blocks = C.c_uint64(99)
    assert lib.dint_score_documents(r.qi._h, r.fd._h, r.wand._h, terms.ctypes.data, offs.ctypes.data, 1, docs2.ctypes.data,
                                    doc_offs2.ctypes.data, scores2.ctypes.data, None, C.byref(blocks), None) == 0
    assert (scores2[:3] == -1.0).all() and np.array_equal(bits(scores2[3:]), bits(want.scores)) and blocks.value == want.blocks_read
    r.close()


@pytest.mark.parametrize("kind", KINDS)
def test_docids_near_2_to_the_32(device, kind):
    """tests/test_gpu_query_high_docids.py's index (lists ending at 0xFFFFFFFE, freqs near 2^32 and wrapped to 0 in full blocks):
    norm_lens covers every docID below 2^32 - 1 (pages of zeros the host never touches but where a posting lies)."""
    rng = np.random.default_rng(77 + kind)
    lists, freqs = _high_lists(rng)
    h = HighIndex(device, kind, lists, freqs)
    num_docs = TOP + 1
    nl = np.zeros(num_docs, dtype=np.float32)
    nl[h.docids] = (rng.random(h.docids.size) * 3 + 0.05).astype(np.float32)
    wand = device.WandData(nl)
    qi = device.QueryIndex(h.dd, h.index, h.offsets)
    bl = ranked.BuilderLists(h.docids, h.freqs, h.bounds)
    n = len(lists)
    qs = [[0], [0, 1], [1, 5, 9], [2, 0], [2, 7], [3, 6], [], list(range(n)), [9, 9, 1], [3, 3]]
    qs += [rng.integers(0, n, int(rng.integers(2, 6))).tolist() for _ in range(10)]
    edge = np.array([0, 1, (1 << 31) - 1, 1 << 31, TOP - 40_001, TOP - 1000, TOP - 1, TOP, 0xFFFFFFFF], dtype=np.uint32)
    docs = []
    for i, q in enumerate(qs):
        u = S.union_of(bl, q)
        d = u if i % 2 == 0 else S.draw_from_union(rng, bl, q, 500)
        docs.append(np.concatenate([d, edge, rng.integers(TOP - 40_000, TOP, 100).astype(np.uint32)]).astype(np.uint32))
    for opts in (dict(), dict(query_or_pass_pages=1), dict(query_or_pass_pages=5)):
        with device.options(**opts):
            got, mods = check(qi, h.fd, wand, bl, nl, num_docs, qs, docs, opts)
    assert any((m.held & (m.freqs == 0)).any() for m in mods), "a wrapped freq of 0 is among the postings scored"
    assert any((m.freqs >= 0xFFFFFFF0).any() for m in mods)
    qi.close()
    wand.close()
