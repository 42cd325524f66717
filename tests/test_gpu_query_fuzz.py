"""Differential fuzzing of the seven query types on the GPU: AND, AND with freqs, OR, OR with freqs, ranked AND, ranked OR
and MaxScore-pruned ranked OR over the query plan of tests/fuzz_streams.py (random dictionary files, random decoder-legal
posting lists of up to 80 pages, wrapped freqs of 0 and freqs near 2^32) — against plain set arithmetic over the generator's
postings, the binary32 models of tests/ranked.py / tests/ranked_or.py, the pruned call's model (tests/maxscore.py: the same
answer as ranked OR and its blocks read, block for block) and on a sample the lists the CPU oracle decodes from the index
bytes. Every case runs a seeded query mix (empty, single-term, repeated-term, 8-32-term, small and large queries in one
call) in one call and, on a sample, one query per call, under a seeded setting of the query options; the pruned call also
with its queries reversed and with every query twice in the call. The draws are tests/query_fuzz_draws.py's, which
tests/test_ranked_or_maxscore_cpu.py replays without a GPU. Then hand-made lists for the ranked selection's edges: ties
across the k-th place over 3, 5, 7 and 33 runs, k = 257 and 1024, scores of 0.0 and subnormal scores."""
import json
import os

import numpy as np
import pytest

import fuzz_streams as F
import maxscore
import ranked
import ranked_or
from dint_amd import host
from or_union import OracleLists, union_freqs
from queries import intersect_freqs
from query_fuzz_draws import CHOICES, KS, NORM_LENS, draw_case, draw_norm_lens, query_mix  # noqa: F401 (the draws live there)

pytestmark = pytest.mark.gpu

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_digests.json")))
QUERY = F.query_plan(*GOLDEN["query_plan"])
assert all(str(c[0]) in GOLDEN["query"] for c in QUERY)


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev

    return dev


@pytest.fixture(autouse=True)
def _options_back_to_default(device):
    yield
    device.reset_options()


def assert_ranked(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what  # bit-equal scores
    assert np.array_equal(got[2], want[2]), what


def ranked_want(fn, lists, qs, nl, num_docs, k):
    out = [fn(lists, q, nl, num_docs, k) for q in qs]
    return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


def run_query_case(device, case, setting=None):
    """Every query type over one case of the query plan (tests/fuzz_soak.py runs this over seeds of its own)."""
    Dd, Df, X = F.build_query_case(case)
    pinned = GOLDEN["query"].get(str(case[0]))
    assert pinned is None or F.index_digest(Dd, Df, X) == pinned["digest"]
    setting, qs, nl, ks = draw_case(case[0], X, setting)
    for k, v in setting.items():
        device.set_option(k, v)
    lens = np.diff(X.bounds)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    qi = device.QueryIndex(dd, X.index, X.offsets)
    uq = [np.unique(np.asarray(q, dtype=np.int64)) for q in qs]
    # AND, AND with freqs
    want_and = [intersect_freqs(X.docids, X.freqs, X.bounds, q) for q in qs]
    want_n = np.array([w[0] for w in want_and], dtype=np.uint64)
    assert int(want_n.sum()) > 0 and int(want_n.max()) > 256, "the mix has AND matches over several pages"
    assert np.array_equal(qi.and_queries(qs), want_n), setting
    counts, sums, _ = qi.and_queries_with_freqs(fd, qs)
    assert np.array_equal(counts, want_n) and np.array_equal(sums, [w[1] for w in want_and]), setting
    # OR, OR with freqs: every freqs part of every distinct term is decoded
    want_or = [union_freqs(X.docids, X.freqs, X.bounds, q) for q in qs]
    want_u = np.array([w[0] for w in want_or], dtype=np.uint64)
    assert np.array_equal(qi.or_queries(qs), want_u), setting
    counts, sums, nblocks = qi.or_queries_with_freqs(fd, qs)
    assert np.array_equal(counts, want_u) and np.array_equal(sums, [w[1] for w in want_or]), setting
    assert nblocks == sum(int(((lens[t] + 255) // 256).sum()) for t in uq), setting
    # ranked AND / OR at two k, over norm_lens of one class
    num_docs = int(X.docids.max()) + 1
    wand = device.WandData(nl)
    lists = ranked.BuilderLists(X.docids, X.freqs, X.bounds)
    wants = {}
    for k in ks:
        for name, fn in (("ranked_and", ranked.ranked_and), ("ranked_or", ranked_or.ranked_or)):
            want = ranked_want(fn, lists, qs, nl, num_docs, k)
            assert_ranked(getattr(qi, name + "_queries")(fd, wand, qs, k=k), want, (name, k, setting))
            wants[name, k] = want
    # pruned ranked OR: ranked OR's answer bit for bit, the blocks read those of the model; the call reversed and with every
    # query twice changes no query's answer (claims are per query, even where two queries of a pass share an N term)
    mtw = ranked.max_term_weights(X.docids, X.freqs, X.bounds, nl)
    mwand = device.WandData(nl, max_term_weight=mtw)
    models = {k: [maxscore.maxscore(lists, q, nl, mtw, num_docs, k) for q in qs] for k in ks}
    for k in ks:
        want, blocks = wants["ranked_or", k], sum(m.blocks_read for m in models[k])
        got = qi.ranked_or_maxscore_queries(fd, mwand, qs, k=k)
        assert_ranked(got[:3], want, ("ranked_or_maxscore", k, setting))
        assert got[3] == blocks, ("ranked_or_maxscore blocks", k, setting)
        got = qi.ranked_or_maxscore_queries(fd, mwand, qs[::-1], k=k)
        assert_ranked(got[:3], tuple(a[::-1] for a in want), ("ranked_or_maxscore reversed", k, setting))
        assert got[3] == blocks, ("ranked_or_maxscore reversed blocks", k, setting)
        got = qi.ranked_or_maxscore_queries(fd, mwand, [q for q in qs for _ in range(2)], k=k)
        assert_ranked(got[:3], tuple(np.repeat(a, 2, axis=0) for a in want), ("ranked_or_maxscore twice", k, setting))
        assert got[3] == 2 * blocks, ("ranked_or_maxscore twice blocks", k, setting)
    # one query per call, on a sample
    sample = list(range(0, len(qs), 7))
    for i in sample:
        q = qs[i]
        assert int(qi.and_queries([q])[0]) == want_and[i][0]
        assert tuple(int(x[0]) for x in qi.and_queries_with_freqs(fd, [q])[:2]) == want_and[i]
        assert int(qi.or_queries([q])[0]) == want_or[i][0]
        assert tuple(int(x[0]) for x in qi.or_queries_with_freqs(fd, [q])[:2]) == want_or[i]
        for name in ("ranked_and", "ranked_or"):
            k = ks[i % 2]
            want = tuple(a[i:i + 1] for a in wants[name, k])
            assert_ranked(getattr(qi, name + "_queries")(fd, wand, [q], k=k), want, (name, k, i))
        k = ks[i % 2]
        got = qi.ranked_or_maxscore_queries(fd, mwand, [q], k=k)
        assert_ranked(got[:3], tuple(a[i:i + 1] for a in wants["ranked_or", k]), ("ranked_or_maxscore", k, i))
        assert got[3] == models[k][i].blocks_read, ("ranked_or_maxscore blocks", k, i)
    # the lists as the oracle decodes them from the index bytes, on a sample
    ol = OracleLists(Dd.kind, Dd.file, Df.file, X.index, X.offsets)
    for i in sample:
        assert ol.union(qs[i]) == want_or[i][0]
        for name, fn in (("ranked_and", ranked.ranked_and), ("ranked_or", ranked_or.ranked_or)):
            want = ranked_want(fn, ol, [qs[i]], nl, num_docs, ks[0])
            assert_ranked(tuple(a[i:i + 1] for a in wants[name, ks[0]]), want, (name, "oracle", i))
        m = maxscore.maxscore(ol, qs[i], nl, mtw, num_docs, ks[0])
        assert_ranked(tuple(a[i:i + 1] for a in wants["ranked_or", ks[0]]),
                      (np.array([m.count], dtype=np.uint64), m.scores[None], m.ids[None]), ("ranked_or_maxscore", "oracle", i))
        assert m.blocks_read == models[ks[0]][i].blocks_read, ("ranked_or_maxscore blocks", "oracle", i)
    qi.close()
    wand.close()
    mwand.close()


@pytest.mark.parametrize("case", QUERY, ids=lambda c: f"seed{c[0]}")
def test_query_case(device, case):
    run_query_case(device, case)


# ---------------------------------------------------------------------------------------------------------------
# the ranked selection's edges, hand-made: ranked_topk cuts a query's candidate slots into runs of R = max(256, next power
# of two >= k) keys, sorts every run, then merges runs pairwise (an odd run count leaves a run over on some passes)
# ---------------------------------------------------------------------------------------------------------------
class HandIndex:
    """Lists built with the project's encoder (host.build_index), norm_lens over num_docs documents."""

    def __init__(self, device, kind, lists, freqs, num_docs, norm_lens):
        self.lens = np.array([x.size for x in lists], dtype=np.uint32)
        self.docids = np.concatenate(lists).astype(np.uint32)
        self.freqs = np.concatenate(freqs).astype(np.uint32)
        self.bounds = np.concatenate([[0], np.cumsum(self.lens)]).astype(np.uint64)
        gaps = np.concatenate([host.docids_to_gaps(x) for x in lists])
        docs_dict = host.build_dictionary(kind, host.Collection(gaps, self.lens))
        freqs_dict = host.build_dictionary(kind, host.Collection(self.freqs - np.uint32(1), self.lens))
        index, offsets = host.build_index(kind, docs_dict, freqs_dict, self.docids, self.freqs, self.lens)
        self.qi = device.QueryIndex(device.Dictionary(kind, docs_dict), index, offsets)
        self.fd = device.Dictionary(kind, freqs_dict)
        self.num_docs, self.nl = num_docs, np.asarray(norm_lens, dtype=np.float32)
        self.wand = device.WandData(self.nl)
        self.lists = ranked.BuilderLists(self.docids, self.freqs, self.bounds)

    def check(self, qs, k, name="ranked_and"):
        fn = ranked.ranked_and if name == "ranked_and" else ranked_or.ranked_or
        want = ranked_want(fn, self.lists, qs, self.nl, self.num_docs, k)
        got = getattr(self.qi, name + "_queries")(self.fd, self.wand, qs, k=k)
        assert_ranked(got, want, (name, k))
        return got

    def close(self):
        self.qi.close()
        self.wand.close()


def _tied_lists(r, runs_pages):
    """Per page count P: a list of P full pages (P runs of 256 slots at R = 256), docIDs 0, 3, 6, ..., freqs 1 but for a
    few freq-2 documents near the end; with equal norm_lens every freq-1 document ties."""
    lists, freqs = [], []
    for pages in runs_pages:
        n = 256 * pages
        lists.append(np.arange(0, 3 * n, 3, dtype=np.uint32))
        f = np.ones(n, dtype=np.uint32)
        f[r.choice(np.arange(n // 2, n), 5, replace=False)] = 2
        freqs.append(f)
    # a list holding every docID of the others and more: AND with it keeps the ties, OR adds tied ones of its own
    lists.append(np.arange(0, 3 * 256 * max(runs_pages), dtype=np.uint32))
    freqs.append(np.ones(lists[-1].size, dtype=np.uint32))
    return lists, freqs


@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
def test_ties_straddle_the_kth_place(device, kind):
    r = np.random.default_rng(4242)
    pages = [3, 5, 7, 33]
    lists, freqs = _tied_lists(r, pages)
    num_docs = int(lists[-1][-1]) + 1
    h = HandIndex(device, kind, lists, freqs, num_docs, np.ones(num_docs, dtype=np.float32))
    whole = len(lists) - 1
    qs = [[t] for t in range(len(pages))] + [[t, whole] for t in range(len(pages))]
    for k in (256, 100, 257, 1024, 1023):
        got = h.check(qs, k)
        for i, t in enumerate(list(range(len(pages))) * 2):
            n = min(k, lists[t].size)
            f2 = np.sort(lists[t][freqs[t] == 2])
            tied = lists[t][freqs[t] == 1][:n - f2.size]  # the smallest docIDs among the tied ones
            assert np.array_equal(got[2][i][:n], np.concatenate([f2, tied])), (k, t)
    # ranked OR: the same ties, one query per pass
    qs_or = [[t, whole] for t in range(len(pages))] + [[0, 1, 2]]
    for pass_pages in (1, 1 << 20):
        with device.options(query_or_pass_pages=pass_pages):
            for k in (256, 257, 1024):
                h.check(qs_or, k, "ranked_or")
                h.check(qs, k, "ranked_or")
    h.close()


def test_freq_zero_scores_zero_and_is_counted(device):
    """A freq of 0 (freq - 1 wraps to 0xFFFFFFFF: a full block only) scores exactly 0.0: the document is counted and comes
    last, equal zeros by ascending docID."""
    kind = host.SINGLE_PACKED
    a = np.arange(0, 2 * 768, 2, dtype=np.uint32)    # 3 full blocks
    b = np.arange(0, 2 * 768, 1, dtype=np.uint32)    # 6 full blocks
    fa = np.full(a.size, 3, dtype=np.uint32)
    zero = np.array([5, 100, 300, 301, 600])
    fa[zero] = 0
    fb = np.ones(b.size, dtype=np.uint32)
    num_docs = int(b[-1]) + 1
    h = HandIndex(device, kind, [a, b], [fa, fb], num_docs, np.ones(num_docs, dtype=np.float32))
    for k in (1024, 768, 766):
        got = h.check([[0], [0, 1]], k)
        assert int(got[0][0]) == min(k, a.size)
        n = min(k, a.size)
        if k >= a.size:  # the zeros last, by ascending docID
            assert np.array_equal(got[2][0][n - zero.size:n], a[zero]) and (got[1][0][n - zero.size:n] == 0).all()
            assert (got[1][0][:n - zero.size] > 0).all()
    for k in (1024, 1000):
        got = h.check([[0], [0, 1]], k, "ranked_or")
        assert int(got[0][0]) == a.size and int(got[0][1]) == min(k, b.size)
    h.close()


def test_subnormal_scores_are_not_flushed(device):
    """norm_lens large enough that q_weight * w (and w itself) is a subnormal binary32: the device keeps them, bit for bit
    as the reference's CPU arithmetic does, and orders by them."""
    kind = host.RECTANGULAR
    r = np.random.default_rng(777)
    n_docs = 1200
    dense = np.arange(0, n_docs, dtype=np.uint32)               # df = num_docs: the clamped idf, q_weight = 2.2e-6
    half = np.sort(r.choice(n_docs, 700, replace=False)).astype(np.uint32)  # df > num_docs / 2: clamped too
    rare = np.sort(r.choice(n_docs, 90, replace=False)).astype(np.uint32)
    lists = [dense, half, rare]
    freqs = [r.integers(1, 20, x.size).astype(np.uint32) for x in lists]
    nl = (r.random(n_docs) + 0.5).astype(np.float32)
    large = r.random(n_docs) < 0.67
    nl[large] = (10.0 ** r.uniform(36, 38.5, int(large.sum()))).astype(np.float32)
    h = HandIndex(device, kind, lists, freqs, n_docs, nl)
    qs = [[0], [1], [0, 1], [0, 2], [1, 2, 2], [0, 1, 2]]
    for name in ("ranked_and", "ranked_or"):
        for k in (10, 1024):
            got = h.check(qs, k, name)
            if k == 1024:
                for i in (0, 2):  # the clamped terms alone: subnormal scores among the first 1024
                    s = got[1][i][:int(got[0][i])]
                    assert ((s > 0) & (s < np.finfo(np.float32).tiny)).sum() > 100, "the test reaches subnormal scores"
    h.close()
