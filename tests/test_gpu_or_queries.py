"""OR queries on the GPU through the C ABI (dint_or_queries, dint_or_queries_freqs): result counts identical to plain set
union of the index builder's input and to the union of the lists the CPU oracle decodes (or_query, include/ds2i/queries.hpp:86-130)."""
import itertools

import numpy as np
import pytest

from dint_amd import host
from or_union import oracle_lists, union, union_freqs
from queries import ReadmeIndex, heavy_queries, intersect, reference_queries
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu


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


def _query_index(device, ix, kind):
    return device.QueryIndex(device.Dictionary(kind, ix.docs_dict), ix.bytes, ix.offsets)


def _unions(ix, qs):
    return np.array([union(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)


def _blocks(ix, terms):
    return sum((int(ix.lens[t]) + 255) // 256 for t in np.unique(np.asarray(terms, dtype=np.int64)))


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_matches_set_union_and_oracle(device, request, kind, corpus_name):
    corpus = request.getfixturevalue(corpus_name)
    ix = get_index(corpus, kind)
    qi = _query_index(device, ix, kind)
    qs = reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 200)
    got = qi.or_queries(qs)
    want = _unions(ix, qs)
    assert np.array_equal(got, want)
    assert int(want.sum()) > 10_000
    ol = oracle_lists(ix, kind)
    for i in range(0, len(qs), 7):
        assert int(got[i]) == ol.union(qs[i])
    qi.close()


def test_edges(device, dense_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(dense_corpus, kind)
    qi = _query_index(device, ix, kind)
    longest, shortest = int(np.argmax(ix.lens)), int(np.argmin(ix.lens))
    assert qi.or_queries([]).size == 0
    assert np.array_equal(qi.or_queries([[], []]), [0, 0])
    got = qi.or_queries([[], [longest], [longest] * 4, [shortest, longest], [shortest], [shortest, longest, shortest]])
    u = union(ix.docids, ix.bounds, [shortest, longest])
    assert list(got) == [0, ix.lens[longest], ix.lens[longest], u, ix.lens[shortest], u]
    with pytest.raises(device.DintError):
        qi.or_queries([[len(ix.lens)]])  # no such list
    with pytest.raises(device.DintError):
        qi.or_queries([[longest], [shortest, len(ix.lens) + 5]])
    qi.close()


def _hand_made(device, kind):
    a = np.arange(0, 3000, dtype=np.uint32)
    b = np.arange(5000, 9000, dtype=np.uint32)               # disjoint, beyond a
    ev = np.arange(0, 20000, 2, dtype=np.uint32)
    od_ = np.arange(1, 20000, 2, dtype=np.uint32)
    sup = np.arange(0, 20000, dtype=np.uint32)
    lists = [a, b, ev, od_, sup, a.copy()]                   # (list 5: the same docIDs as list 0)
    docids = np.concatenate(lists)
    lens = np.array([len(x) for x in lists], dtype=np.uint32)
    gaps = np.concatenate([host.docids_to_gaps(x) for x in lists])
    coll = host.Collection(gaps, lens)
    freqs = (np.arange(docids.size, dtype=np.uint32) % 5) + 1
    dd = host.build_dictionary(kind, coll)
    fd = host.build_dictionary(kind, host.Collection(freqs - 1, lens))
    idx, offs = host.build_index(kind, dd, fd, docids, freqs, lens)
    qi = device.QueryIndex(device.Dictionary(kind, dd), idx, offs)
    return qi, device.Dictionary(kind, fd), lists, freqs, lens


def test_disjoint_identical_interleaved_and_superset_lists(device):
    """Disjoint ranges (every probe past the last block), identical lists (every probe hits), evens and odds (every probe
    lands in a block and misses), a list with a superset of it."""
    qi, fd, lists, freqs, lens = _hand_made(device, host.SINGLE_PACKED)
    qs = [[0, 1], [1, 0], [0, 5], [5, 0, 5], [2, 3], [3, 2], [2, 4], [4, 2], [3, 4, 2], [0, 2, 3], [1, 3, 5]]
    want = [len(np.unique(np.concatenate([lists[t] for t in set(q)]))) for q in qs]
    assert want[:4] == [7000, 7000, 3000, 3000] and want[4] == 20000
    assert list(qi.or_queries(qs)) == want
    counts, sums, nblocks = qi.or_queries_with_freqs(fd, qs)
    bounds = np.concatenate([[0], np.cumsum(lens.astype(np.int64))]).astype(np.int64)
    assert list(counts) == want
    assert list(sums) == [sum(int(freqs[bounds[t]:bounds[t + 1]].sum()) for t in set(q)) for q in qs]
    assert nblocks == sum(sum((int(lens[t]) + 255) // 256 for t in set(q)) for q in qs)
    qi.close()


def test_term_order_does_not_matter(device, small_corpus):
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    qi = _query_index(device, ix, kind)
    order = np.argsort(-ix.lens.astype(np.int64), kind="stable")
    bases = [[order[0], order[1], order[5]], [order[2], order[40], order[300], order[7]], [order[3], order[3], order[900]]]
    for base in bases:
        perms = [list(p) for p in itertools.permutations(base)]
        got = qi.or_queries(perms)
        assert set(int(g) for g in got) == {union(ix.docids, ix.bounds, base)}
    qi.close()


def test_batch_equals_one_query_per_call(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    qi = _query_index(device, ix, kind)
    qs = heavy_queries(ix.lens, 40, seed=9)
    batch = qi.or_queries(qs)
    assert np.array_equal(batch, _unions(ix, qs))
    for q, want in zip(qs, batch):
        assert int(qi.or_queries([q])[0]) == int(want)
    assert np.array_equal(qi.or_queries(qs), batch)
    qi.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_a_call_in_many_passes(device, small_corpus, kind, pass_pages):
    """query_or_pass_pages bounds the pages a pass decodes: a call cut into many passes, and queries larger than the bound
    (each alone in a pass of its own size), give what one pass gives."""
    ix = get_index(small_corpus, kind)
    dd, fd = device.Dictionary(kind, ix.docs_dict), device.Dictionary(kind, ix.freqs_dict)
    qi = device.QueryIndex(dd, ix.bytes, ix.offsets)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2)
    assert max(_blocks(ix, q) for q in qs) > 7
    one_counts, one_sums, one_blocks = qi.or_queries_with_freqs(fd, qs)
    one = qi.or_queries(qs)
    device.set_option("query_or_pass_pages", pass_pages)
    assert np.array_equal(qi.or_queries(qs), one)
    counts, sums, nblocks = qi.or_queries_with_freqs(fd, qs)
    assert np.array_equal(counts, one_counts) and np.array_equal(sums, one_sums) and nblocks == one_blocks
    assert np.array_equal(one, _unions(ix, qs))
    qi.close()


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus"])
def test_with_freqs(device, request, kind, corpus_name):
    """or_query<true>: the freq of every posting of every distinct term is read, so every freqs part is decoded."""
    corpus = request.getfixturevalue(corpus_name)
    ix = get_index(corpus, kind)
    dd, fd = device.Dictionary(kind, ix.docs_dict), device.Dictionary(kind, ix.freqs_dict)
    qi = device.QueryIndex(dd, ix.bytes, ix.offsets)
    qs = reference_queries(len(ix.lens))[:150] + heavy_queries(ix.lens, 120, seed=11)
    counts, sums, nblocks = qi.or_queries_with_freqs(fd, qs)
    want = [union_freqs(ix.docids, ix.freqs, ix.bounds, q) for q in qs]
    assert np.array_equal(counts, np.array([w[0] for w in want], dtype=np.uint64))
    assert np.array_equal(sums, np.array([w[1] for w in want], dtype=np.uint64))
    assert np.array_equal(counts, qi.or_queries(qs))
    assert nblocks == sum(_blocks(ix, q) for q in qs)
    assert int(sums.sum()) > int(counts.sum()) > 10_000
    qi.close()


def test_with_freqs_edges(device, dense_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(dense_corpus, kind)
    dd, fd = device.Dictionary(kind, ix.docs_dict), device.Dictionary(kind, ix.freqs_dict)
    qi = device.QueryIndex(dd, ix.bytes, ix.offsets)
    c, s, b = qi.or_queries_with_freqs(fd, [])
    assert c.size == 0 and s.size == 0 and b == 0
    c, s, b = qi.or_queries_with_freqs(fd, [[], []])
    assert list(c) == [0, 0] and list(s) == [0, 0] and b == 0
    big, small = int(np.argmax(ix.lens)), int(np.argmin(ix.lens))
    c, s, b = qi.or_queries_with_freqs(fd, [[big], [big] * 4, [], [small, big]])
    lo, hi = int(ix.bounds[big]), int(ix.bounds[big + 1])
    fbig = int(ix.freqs[lo:hi].astype(np.uint64).sum())
    assert list(c) == [hi - lo, hi - lo, 0, union(ix.docids, ix.bounds, [small, big])]
    assert list(s) == [fbig, fbig, 0, union_freqs(ix.docids, ix.freqs, ix.bounds, [small, big])[1]]
    assert b == 2 * _blocks(ix, [big]) + _blocks(ix, [small, big])
    with pytest.raises(device.DintError):
        qi.or_queries_with_freqs(fd, [[len(ix.lens)]])
    wrong = device.Dictionary(host.RECTANGULAR, get_index(dense_corpus, host.RECTANGULAR).freqs_dict)
    with pytest.raises(device.DintError):
        qi.or_queries_with_freqs(wrong, [[big]])
    qi.close()


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.MULTI_PACKED])
def test_reference_query_log_on_the_readme_shaped_collection(device, kind):
    """The reference's query log, term ids as they are, over the README-shaped collection: batched and one query per call."""
    ix = ReadmeIndex(kind)
    qs = reference_queries(len(ix.lens))
    dd, fd = device.Dictionary(kind, ix.docs_dict), device.Dictionary(kind, ix.freqs_dict)
    qi = device.QueryIndex(dd, ix.bytes, ix.offsets)
    want = _unions(ix, qs)
    assert np.array_equal(qi.or_queries(qs), want) and int(want.sum()) > 10_000
    counts, sums, _ = qi.or_queries_with_freqs(fd, qs)
    wf = [union_freqs(ix.docids, ix.freqs, ix.bounds, q) for q in qs]
    assert np.array_equal(counts, want) and np.array_equal(sums, np.array([w[1] for w in wf], dtype=np.uint64))
    for i in range(0, len(qs), 11):
        assert int(qi.or_queries([qs[i]])[0]) == int(want[i])
    qi.close()


@pytest.mark.parametrize("batch_fused", [1, 0])
def test_and_calls_around_or_calls(device, small_corpus, batch_fused):
    """One query index for both: AND, then OR, then AND again — the AND results do not change (an OR call leaves the
    claim flags and tables, and the workspaces it shares, fit for the next AND call). Small queries (the workgroup-per-query
    form, or with query_batch_fused = 0 the round-per-launch form) and a mixed batch."""
    device.set_option("query_batch_fused", batch_fused)
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    qi = _query_index(device, ix, kind)
    every = reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 60, seed=3)
    small = [q for q in every if len(set(q)) >= 2 and min(int(ix.lens[t]) for t in q) <= 16 * 256][:300]
    mixed = every[:200]
    want_small = np.array([intersect(ix.docids, ix.bounds, q) for q in small], dtype=np.uint64)
    want_mixed = np.array([intersect(ix.docids, ix.bounds, q) for q in mixed], dtype=np.uint64)
    assert np.array_equal(qi.and_queries(small), want_small)
    assert np.array_equal(qi.and_queries(mixed), want_mixed)
    assert np.array_equal(qi.or_queries(every), _unions(ix, every))
    assert np.array_equal(qi.and_queries(small), want_small)
    assert int(qi.and_queries([mixed[-1]])[0]) == int(want_mixed[-1])
    assert np.array_equal(qi.or_queries(small), _unions(ix, small))
    assert np.array_equal(qi.and_queries(mixed), want_mixed)
    qi.close()


def test_one_query_index_under_two_host_threads(device, small_corpus):
    """Two host threads, a stream each, one calling or_queries and the other and_queries on the same query index: the calls
    serialise on the handle's lock, every result is right."""
    import threading
    import time

    import torch

    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    qi = _query_index(device, ix, kind)
    light = reference_queries(len(ix.lens))[:200]
    heavy = heavy_queries(ix.lens, 30, seed=11)
    qs = light[:60] + heavy
    want_or = _unions(ix, qs)
    want_and = np.array([intersect(ix.docids, ix.bounds, q) for q in qs], dtype=np.uint64)
    errors, calls = [], [0, 0]
    stop_at = time.monotonic() + 4.0

    def worker(k):
        try:
            stream = torch.cuda.Stream(torch.device("cuda", 0))
            r = np.random.default_rng(200 + k)
            call = qi.or_queries_packed if k == 0 else qi.and_queries_packed
            want = want_or if k == 0 else want_and
            terms_all, offs_all = device._pack_queries(qs)
            while time.monotonic() < stop_at:
                if r.integers(0, 2):
                    c = np.zeros(len(qs), dtype=np.uint64)
                    call(terms_all, offs_all, c, stream.cuda_stream)
                    assert np.array_equal(c, want), ("batch", k)
                else:
                    i = int(r.integers(0, len(qs)))
                    t, o = device._pack_queries([qs[i]])
                    c = np.zeros(1, dtype=np.uint64)
                    call(t, o, c, stream.cuda_stream)
                    assert int(c[0]) == int(want[i]), ("one", k, i)
                calls[k] += 1
        except BaseException as e:  # noqa: BLE001 (reported by the main thread)
            errors.append((k, repr(e)))

    threads = [threading.Thread(target=worker, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert min(calls) >= 10, calls
    qi.close()
