"""Collapsed ranked queries on the GPU through the C ABI (dint_ranked_or_collapsed_queries, dint_ranked_and_collapsed_queries;
DESIGN.md 4d-collapse): counts, BM25 scores, docIDs, matches, collapsed, hit_groups and hit_group_matches equal to the model's
(tests/collapse.py: one lexsort of the model's matches by (-score, docID), the first document of every group plus every
document in no group), bit for bit; the facet rows, matches and blocks_decoded equal to the faceted entry's on the same
arguments; and the identities with the faceted and the filtered entries under the maps that make collapsing a no-op or leave
one hit. No tolerance anywhere."""
import ctypes as C
import threading

import numpy as np
import pytest

import collapse as CO
import doc_filter as DF
import facets as FA
import ranked
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import BOTH_FORMS, HAND_DOCS, MAP_MAX_DOCS, Faceted
from test_gpu_facets import hand_maps as facet_hand_maps
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import _hand_made
from test_gpu_ranked_range import HAND_QUERIES
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]
ENTRIES = ("or", "and")
NONE32 = CO.DEVICE_NONE


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


class Collapsed(Faceted):
    """Faceted (an index, its freqs dictionary and wand data on the device, the filtered and faceted entries and the model's
    matches) with the two collapsed entries and their model."""

    def run_c(self, entry, qs, facets, f, k, stats=True, rows=True):
        """-> (counts, scores, docids, matches, blocks_decoded, collapsed, hit_groups, hit_group_matches, rows); without the
        stats no matches and blocks_decoded, without the rows no rows"""
        fn = self.qi.ranked_or_collapsed_queries if entry == "or" else self.qi.ranked_and_collapsed_queries
        return fn(self.fd, self.wand, qs, facets, filter=f, k=k, with_stats=stats, with_rows=rows)

    def want_c(self, entry, qs, mask, group_of, n_groups, k):
        """the model's (counts, scores, docids, matches, collapsed, hit_groups, hit_group_matches, rows)"""
        return CO.stacked([CO.collapse(self.matches_of(entry, q), mask, group_of, n_groups, k) for q in qs], k, n_groups)

    def check_c(self, entry, qs, group_of, n_groups, k=10, mask=None, f=None, facets=None, what=None, faceted=True):
        """the collapsed call (through the handles given, or ones made and closed here) against the model, bit for bit, and —
        faceted — its matches, blocks_decoded and rows against the faceted entry on the same arguments"""
        what = (entry, n_groups, k, what)
        own_f, own_x = f is None and mask is not None, facets is None
        if own_f:
            f = self.filter(mask)
        if own_x:
            facets = self.facets(group_of, n_groups)
        got = self.run_c(entry, qs, facets, f, k)
        want = self.want_c(entry, qs, mask, group_of, n_groups, k)
        _bit_equal(got[:4] + got[5:], want, what)
        assert np.array_equal(got[0], np.minimum(got[5], k)) and (got[5] <= got[3]).all(), what
        if faceted:
            same = self.run_x(entry, qs, facets, f, k)
            _bit_equal((got[3], got[8]), (same[3], same[5]), what)
            assert got[4] == same[4], what
        short = self.run_c(entry, qs, facets, f, k, stats=False, rows=False)  # (without the stats and the rows: the same)
        assert len(short) == 6, what
        _bit_equal(short, got[:3] + got[5:8], what)
        if own_f:
            f.close()
        if own_x:
            facets.close()
        return got


@pytest.fixture(scope="module")
def hand(device):
    """test_gpu_ranked_range.py's hand-made index: a = 0 .. 2999 (blocks [256 j, 256 j + 255], the last one 2816 .. 2999),
    b = 5000 .. 8999 (the last block is 8840 .. 8999; 5000 .. 5006 have freq 3, every other posting freq 1), c = the evens,
    d = every doc (page j holds 256 j .. 256 j + 255: a document's lane is d & 63), e = {10, 20, 30, 40}; norm_lens all 1, so
    a document's score is decided by the lists that hold it: equal scores abound, and the smaller docID wins them."""
    kind = host.MULTI_PACKED
    r = Collapsed(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    yield r
    r.close()


# ---- kernel edges on the hand-made index --------------------------------------------------------------------------------
def hand_maps(n_groups):
    """test_gpu_facets.py's hand-made maps (runs that end at lanes 62 | 63, at 63 | 64 and at the page's last slot, group 0
    in lane 0, the last group, a NONE document between two of one group, short maps, the short last blocks, the list of one
    block ...) and the ones collapsing is about. Under [3, 4] and [2, 3, 4] the documents 10, 20, 30, 40 score highest (d's
    pages hold the union's representatives: a document's lane is still d & 63); under [2, 3, 4] the evens score above the
    odds; under [1] the documents 5000 .. 5006 score highest, under [0, 1] a's documents score above b's (a is the rarer list);
    under [3] every score is equal."""
    last = n_groups - 1
    d = np.arange(HAND_DOCS, dtype=np.int64)
    maps = dict(facet_hand_maps(n_groups))
    where = np.full(HAND_DOCS, FA.NONE, dtype=np.int64)
    where[10:16] = 1      # under [3, 4] the best, 10, in the run's first lane
    where[17:24] = 2      # ... 20, in a middle lane
    where[26:31] = last   # ... 30, in the run's last lane
    where[35:46] = 0      # ... 40, in a middle lane, group 0
    where[60:64] = 3      # a run that ends with its wave; under [2, 3, 4] its best is 60, under [3] too
    where[64:70] = 3      # ... and goes on in the next wave: the same group from two waves of one page
    where[250:262] = 4    # ... and from two pages
    maps["the best in the first, a middle and the last lane of its run"] = where
    maps["two equal best scores in one run"] = np.where((d >= 5) & (d < 26), 1, FA.NONE)          # 10 and 20 under [3, 4]: 10 wins
    maps["two equal best scores in two waves of a page"] = np.where((d >= 30) & (d < 101), 2, last)  # 30, 40 | 64 ...
    maps["groups of a hundred documents"] = (d // 100) % n_groups                                 # runs across waves and pages
    maps["groups of a hundred documents, from the top"] = last - (d // 100) % n_groups
    maps["one group over the pages of two terms"] = np.where((d >= 2900) & (d < 5100), last, (d // 500) % n_groups)  # a's and b's under [0, 1]
    maps["every document its own run, two groups"] = d & 1
    maps["one group"] = FA.named_map("one group", HAND_DOCS, n_groups)
    return maps


HAND_MAP_NAMES = list(hand_maps(300))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_groups", BOTH_FORMS)
@pytest.mark.parametrize("name", HAND_MAP_NAMES)
def test_kernel_edges(hand, entry, n_groups, name):
    """HAND_QUERIES under every hand-made map. Among them [3] (full pages of consecutive documents, every score equal), [3, 4]
    and [2, 3, 4] (a few documents above the others), [0] and [1] (short last blocks), [4] (a list of one block), [0, 1] (a
    group over the pages of two terms, OR) and — a dead slot between two live ones of one group — [0, 2] and [1, 2, 3]."""
    g = hand_maps(n_groups)[name]
    x = hand.facets(g, n_groups)
    got = hand.check_c(entry, HAND_QUERIES, g, n_groups, k=10, facets=x, what=name)
    for i in (2, 3, 5, 7, 9, 10, 14):  # one query per call: the same answer, a deeper k the same prefix
        one = hand.check_c(entry, [HAND_QUERIES[i]], g, n_groups, k=1000, facets=x, what=(name, i), faceted=False)
        assert one[5][0] == got[5][i] and one[3][0] == got[3][i]
        for j in (1, 2, 6, 7):
            assert np.asarray(one[j][0][:10]).tobytes() == np.asarray(got[j][i]).tobytes(), (name, i, j)
    x.close()


def test_the_edge_cases_are_what_they_are_said_to_be(hand):
    n_groups = 257
    maps = hand_maps(n_groups)
    last = n_groups - 1

    def hits(entry, q, name, k=10, mask=None):
        w = hand.want_c(entry, [q], mask, maps[name], n_groups, k)
        return {int(g): (int(d), int(n)) for g, d, n in zip(w[5][0], w[2][0], w[6][0]) if g != NONE32}, w

    # the best of a run in its first, a middle and its last lane; a group met from two waves and from two pages
    by_group, w = hits("or", [3, 4], "the best in the first, a middle and the last lane of its run", k=1000)
    assert by_group[1] == (10, 6) and by_group[2] == (20, 7) and by_group[last] == (30, 5) and by_group[0] == (40, 11)
    assert by_group[3] == (60, 10) and by_group[4] == (250, 12)
    assert w[2][0][:4].tolist() == [10, 20, 30, 40] and w[4][0] == 9000 - 51 + 6  # 51 grouped documents in 6 groups
    by_group, _ = hits("or", [2, 3, 4], "the best in the first, a middle and the last lane of its run", k=1000)
    assert by_group[3] == (60, 10) and by_group[4] == (250, 12) and by_group[2] == (20, 7)
    # two equal best scores: the smaller docID wins — in one run, in two waves of a page, in two pages
    by_group, w = hits("or", [3, 4], "two equal best scores in one run", k=3)
    assert by_group == {1: (10, 21)} and w[2][0].tolist() == [10, 30, 40]  # (30 and 40 are in no group)
    by_group, _ = hits("or", [3, 4], "two equal best scores in two waves of a page")
    assert by_group == {2: (30, 71), last: (10, 9000 - 71)}
    by_group, _ = hits("or", [3], "two equal best scores in two waves of a page")
    assert by_group == {2: (30, 71), last: (0, 9000 - 71)}
    by_group, w = hits("or", [3], "groups of a hundred documents", k=1000)
    assert w[4][0] == 90 and all(by_group[g] == (100 * g, 100) for g in range(90))  # (group 2: 200 .. 299, pages 0 and 1)
    # one group over the pages of two terms: a's last page holds 2900 .. 2999, b's first 5000 .. 5099; a is the rarer list,
    # so its documents score above b's, and both pages offer the group a best
    by_group, _ = hits("or", [0, 1], "one group over the pages of two terms", k=20)
    assert by_group[last] == (2900, 200)
    sc, ids = hand.matches_of("or", [0, 1])
    assert sc[ids == 2900][0] > sc[ids == 5000][0] > sc[ids == 5099][0]
    # the dead slot between two live ones: in a's pages the union of [0, 2] has every other slot dead, and so has the
    # intersection; a group still keeps exactly one document
    for entry in ENTRIES:
        w = hand.want_c(entry, [[0, 2]], None, maps["clustered"], n_groups, 1000)
        assert w[4][0] == len(set(maps["clustered"][hand.matches_of(entry, [0, 2])[1]].tolist()))
    # a NONE document between two of one group: it is kept beside the group's best
    w = hand.want_c("or", [[3]], None, maps["a NONE document between two of one group"], n_groups, 10)
    assert w[2][0][:6].tolist() == [0, 100, 101, 127, 128, 2999] and w[4][0] == 6 and w[5][0][:2].tolist() == [3, NONE32]
    assert w[6][0][:6].tolist() == [8995, 1, 1, 1, 1, 1] and w[0][0] == 6
    # a map that ends below the largest match: the documents past it are all kept
    for name, n_map in (("the map ends inside a page", 5100), ("the map ends before the first match of b", 300), ("a map of one document", 1)):
        for entry in ENTRIES:
            got = hand.check_c(entry, HAND_QUERIES, maps[name], n_groups, what=name)
            ids = [hand.matches_of(entry, q)[1] for q in HAND_QUERIES]
            past = np.array([int((d >= n_map).sum()) for d in ids])
            groups_inside = np.array([len(set(maps[name][d[d < n_map]].tolist()) - {FA.NONE}) for d in ids])
            assert np.array_equal(got[5].astype(np.int64), past + groups_inside) and past.sum() > 0
    # the last group and group 0
    by_group, _ = hits("or", [3], "a run ends at lane 63, the next begins a wave")
    assert by_group == {0: (0, 64), last: (64, 9000 - 64)}


@pytest.mark.parametrize("entry", ENTRIES)
def test_edges_under_a_filter(hand, entry):
    """the filter path: pages are the live blocks, and what they hold outside the filter is dead before the best is taken —
    the best document of a group outside the filter: the best inside wins"""
    for members in ([63, 64, 65], list(range(200, 600)) + [2999, 8999], list(range(0, HAND_DOCS, 3)),
                    [d for d in range(HAND_DOCS) if d not in (10, 30, 2900, 2901)]):
        mask = DF.as_mask(members, HAND_DOCS)
        f = hand.filter(mask)
        for n_groups in BOTH_FORMS:
            for name in ("a run ends at lane 63, the next begins a wave", "two equal best scores in one run", "clustered",
                         "the best in the first, a middle and the last lane of its run", "one group over the pages of two terms",
                         "every other document NONE", "the map ends inside a page"):
                hand.check_c(entry, HAND_QUERIES, hand_maps(n_groups)[name], n_groups, mask=mask, f=f, what=(name, len(members)))
        f.close()
    # without 10 the group of 5 .. 25 is shown by 20, without 2900 and 2901 the group over two terms by 2902
    mask = DF.as_mask([d for d in range(HAND_DOCS) if d not in (10, 30, 2900, 2901)], HAND_DOCS)
    got = hand.check_c("or", [[3, 4], [0, 1]], hand_maps(257)["two equal best scores in one run"], 257, mask=mask, k=3)
    assert got[2][0].tolist() == [20, 40, 0] and got[7][0].tolist() == [20, 1, 1] and got[6][0].tolist() == [1, NONE32, NONE32]
    got = hand.check_c("or", [[0, 1]], hand_maps(257)["one group over the pages of two terms"], 257, mask=mask, k=20)
    at = got[6][0].tolist().index(256)
    assert got[2][0][at] == 2902 and got[7][0][at] == 198 and got[5][0] == 15  # (groups 0 .. 5 and 10 .. 17, and the one over two terms)


@pytest.mark.parametrize("entry", ENTRIES)
def test_maps_that_make_collapsing_a_no_op_or_leave_one_hit(hand, entry):
    """Map "none", and every document its own group (9 000 groups): the faceted call's answer, bit for bit, and collapsed ==
    matches. "One group": exactly one hit, the filtered call's top 1, with hit_group_matches == matches. The rows are the
    faceted entry's throughout."""
    mask = DF.as_mask(list(range(0, HAND_DOCS, 3)), HAND_DOCS)
    f = hand.filter(mask)
    for g, n_groups in ((FA.named_map("none", HAND_DOCS, 256), 256), (np.arange(HAND_DOCS, dtype=np.int64), HAND_DOCS)):
        x = hand.facets(g, n_groups)
        for filt, m in ((None, None), (f, mask)):
            for k in (10, 1000):
                got = hand.check_c(entry, HAND_QUERIES, g, n_groups, k=k, mask=m, f=filt, facets=x)
                same = hand.run_x(entry, HAND_QUERIES, x, filt, k)
                _bit_equal(got[:4], same[:4], (entry, n_groups, k))
                _bit_equal((got[8],), (same[5],))
                assert got[4] == same[4] and np.array_equal(got[5], got[3])
        x.close()
    for n_groups in BOTH_FORMS + (1,):
        g = FA.named_map("one group", HAND_DOCS, n_groups)
        x = hand.facets(g, n_groups)
        for filt, m in ((None, None), (f, mask)):
            got = hand.check_c(entry, HAND_QUERIES, g, n_groups, k=10, mask=m, f=filt, facets=x)
            top1 = hand.run_f(entry, HAND_QUERIES, filt, 1)
            some = got[3] > 0
            assert np.array_equal(got[0], some.astype(np.uint64)) and np.array_equal(got[5], got[0]) and some.sum() >= 8
            assert np.array_equal(got[1][:, 0].view(np.uint32), top1[1][:, 0].view(np.uint32)) and np.array_equal(got[2][:, 0], top1[2][:, 0])
            assert np.array_equal(got[7][:, 0].astype(np.uint64), got[3]) and not got[7][:, 1:].any()
            assert (got[6][some, 0] == n_groups - 1).all() and (got[6][~some] == NONE32).all() and (got[6][:, 1:] == NONE32).all()
        x.close()
    f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, entry):
    g = np.arange(HAND_DOCS, dtype=np.int64) // 2 % 3000
    x = hand.facets(g, 3000)
    for k in (1, 1024):
        got = hand.check_c(entry, HAND_QUERIES, g, 3000, k=k, facets=x)
    assert int(got[0].max()) == 1024 and int(got[5].max()) > 1024 and int(got[3].max()) > int(got[5].max())
    x.close()


def test_two_calls_in_a_row_leave_no_stale_bests(hand):
    """one index, different batches: a longer batch first, then shorter ones, other group counts in between — a best key, a
    counter or a hit that the second call did not clear would show. Two queries of a batch that hit the same groups keep
    their own tables."""
    g8, g300 = FA.named_map("striped", HAND_DOCS, 8), FA.named_map("clustered", HAND_DOCS, 300)
    x8, x300 = hand.facets(g8, 8), hand.facets(g300, 300)
    for entry in ENTRIES:
        hand.check_c(entry, HAND_QUERIES, g8, 8, facets=x8)
        hand.check_c(entry, [[4], [], [0, 1]], g8, 8, facets=x8)
        hand.check_c(entry, HAND_QUERIES[::-1], g300, 300, facets=x300)
        hand.check_c(entry, [[], []], g300, 300, facets=x300)
        got = hand.check_c(entry, [[4]], g8, 8, facets=x8)
        assert got[2][0][:4].tolist() == [10, 20, 30, 40] and got[6][0][:5].tolist() == [2, 4, 6, 0, NONE32] and got[5][0] == 4
        # the same groups from several queries of one batch: [3] and [3, 4] and [3] again, and an empty query between them
        got = hand.check_c(entry, [[3], [3, 4], [], [3], [2, 3, 4]], g300, 300, k=300, facets=x300)
        assert got[5].tolist()[:4] == ([300, 300, 0, 300] if entry == "or" else [300, 2, 0, 300])
        assert not got[0][2] and (got[6][2] == NONE32).all() and not got[7][2].any()
    x8.close()
    x300.close()


# ---- the batch ----------------------------------------------------------------------------------------------------------
_EVERY = {}  # {corpus: {(entry, query): every match}}: the model's matches, shared by the three kinds


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_matches():
    yield
    _EVERY.clear()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_is_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Collapsed(device, ix, kind, every=_EVERY.setdefault(corpus_name, {}))
    qs = reference_queries(len(ix.lens))[::4] + heavy_queries(ix.lens, 10) + [[]]
    n_map = min(r.num_docs, MAP_MAX_DOCS)
    mask = DF.batch_filter("runs", DF.batch_num_docs(r.num_docs), ix.docids, None)
    f = r.filter(mask)
    removed = {e: 0 for e in ENTRIES}
    for name in FA.MAPS:
        for n_groups in (8, 1000):
            g = FA.named_map(name, n_map, n_groups)
            x = r.facets(g, n_groups)
            for entry in ENTRIES:
                got = r.check_c(entry, qs, g, n_groups, facets=x, what=(corpus_name, name))
                removed[entry] += int((got[3] - got[5]).sum())
                assert got[5][-1] == 0 and got[3][-1] == 0 and (got[6][-1] == NONE32).all()  # the empty query inside the batch
                r.check_c(entry, qs, g, n_groups, mask=mask, f=f, facets=x, what=(corpus_name, name, "runs"), faceted=False)
            x.close()
    f.close()
    assert removed["or"] > 5000 and removed["and"] > 100, removed
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: a pass holds whole queries, the table of best keys, the counters and
    the hits of the queries of later passes lie at their own offset, and all of them were cleared once."""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Collapsed(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2) + [[], [0]]
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    device.set_option("query_or_pass_pages", pass_pages)
    for n_groups, name in ((8, "clustered"), (1000, "striped")):
        g = FA.named_map(name, r.num_docs, n_groups)
        x = r.facets(g, n_groups)
        for entry in ENTRIES:
            got = r.check_c(entry, qs, g, n_groups, facets=x, what=name)
            back = r.run_c(entry, qs[::-1], x, None, 10)
            for j in (0, 1, 2, 3, 5, 6, 7, 8):
                assert np.asarray(back[j][::-1]).tobytes() == np.asarray(got[j]).tobytes(), (name, entry, j)
            r.check_c(entry, qs, g, n_groups, mask=mask, f=f, facets=x, what=(name, "runs"), faceted=False)
        assert int(got[5][len(qs) // 2:].sum()) > 0  # (queries of later passes keep something)
        x.close()
    f.close()
    r.close()


# ---- docIDs at the top of the u32 range ---------------------------------------------------------------------------------
def test_docids_near_2_to_the_32(device):
    """An index with docIDs up to 0xFFFFFFFE: the key's low word is the inverted docID, 1 for the largest one, and a map that
    ends far below leaves every high document in no group — the map is never read past its end."""
    kind = host.SINGLE_PACKED
    lists = [np.arange(TOP - 599, TOP + 1, dtype=np.uint64).astype(np.uint32), np.array([0, 5, TOP], dtype=np.uint32),
             np.concatenate([np.arange(0, 300, 3, dtype=np.uint64), np.arange(TOP - 298, TOP + 1, 2, dtype=np.uint64)]).astype(np.uint32),
             np.arange((1 << 31) - 300, (1 << 31) + 300, dtype=np.uint64).astype(np.uint32)]
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 9, x.size).astype(np.uint32) for x in lists]
    h = HighIndex(device, kind, lists, freqs)
    num_docs = TOP + 1
    nl = np.zeros(num_docs, dtype=np.float32)  # (pages of zeros the host never touches but where a posting lies)
    nl[h.docids] = (rng.random(h.docids.size) * 3 + 0.05).astype(np.float32)
    qi, wand = device.QueryIndex(h.dd, h.index, h.offsets), device.WandData(nl)
    bl = ranked.BuilderLists(h.docids, h.freqs, h.bounds)
    qs = [[0], [1], [0, 1], [0, 2], [1, 2], [0, 1, 2], [2, 2, 1], [3], [0, 3], [1, 3], []]
    every = {conj: [CO.every_match(bl, q, nl, num_docs, conj) for q in qs] for conj in (False, True)}
    for n_map, n_groups, name in ((100, 7, "striped"), (6, 300, "striped"), (1000, 256, "clustered"), (1, 1, "one group")):
        g = FA.named_map(name, n_map, n_groups)
        x = device.DocFacets(0, g, n_groups)
        for entry in ENTRIES:
            fn = qi.ranked_or_collapsed_queries if entry == "or" else qi.ranked_and_collapsed_queries
            got = fn(h.fd, wand, qs, x, k=10, with_stats=True, with_rows=True)
            want = CO.stacked([CO.collapse(e, None, g, n_groups, 10) for e in every[entry == "and"]], 10, n_groups)
            _bit_equal(got[:4] + got[5:], want, (n_map, entry))
            assert (got[5].astype(np.int64) >= [int((e[1] >= n_map).sum()) for e in every[entry == "and"]]).all()
        x.close()
    qi.close()
    wand.close()


# ---- errors, and two threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, entry):
    lib = device._lib
    call = getattr(lib, f"dint_ranked_{entry}_collapsed_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    g = FA.named_map("striped", HAND_DOCS, 8)
    x = hand.facets(g, 8)

    def attempt(k, terms_, filt, fac, null=(), offs_=offs, n=1):
        """null: the outputs passed as null pointers -> (status, every output still holds its canary)"""
        out = {"counts": np.full(1, 77, dtype=np.uint64), "matches": np.full(1, 77, dtype=np.uint64), "collapsed": np.full(1, 77, dtype=np.uint64),
               "scores": np.full(1025, -1.0, dtype=np.float32), "docids": np.full(1025, 77, dtype=np.uint32),
               "hit_groups": np.full(1025, 77, dtype=np.uint32), "hit_group_matches": np.full(1025, 77, dtype=np.uint32),
               "rows": np.full(16, 77, dtype=np.uint32)}
        blocks = C.c_uint64(77)
        p = {name: None if name in null else a.ctypes.data for name, a in out.items()}
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  fac._h if fac is not None else None, n, p["counts"], p["matches"], p["collapsed"], p["scores"], p["docids"], p["hit_groups"],
                  p["hit_group_matches"], p["rows"], C.byref(blocks), None)
        untouched = all((a == (-1.0 if name == "scores" else 77)).all() for name, a in out.items()) and blocks.value == 77
        return st, untouched

    for filt in (None, f):
        assert attempt(0, terms, filt, x) == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, x) == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 5], dtype=np.uint32), filt, x) == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, x, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)  # decreasing offsets
        assert attempt(10, terms, filt, None) == (DINT_ERR_ARG, True)  # no facets
        for name in ("counts", "scores", "collapsed", "hit_groups", "hit_group_matches"):
            assert attempt(10, terms, filt, x, null=(name,)) == (DINT_ERR_ARG, True), name
    assert attempt(10, terms, f_other, x) == (DINT_ERR_ARG, True)  # a filter of another query index
    # n_queries * n_groups past 2^27: refused before the offsets are read (2^27 itself is not refused for its size)
    big = hand.facets(np.zeros(1, dtype=np.int64), 65536)
    assert attempt(10, terms, None, big, n=(1 << 11) + 1) == (DINT_ERR_ARG, True)
    big.close()
    st, untouched = attempt(10, terms, f, x)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_c(entry, [[5]], x, f, 10)
    with pytest.raises(device.DintError):
        hand.run_c(entry, [[0]], x, f_other, 10)
    # nullable outputs: matches, docids, facet_counts and blocks_decoded
    st, _ = attempt(10, terms, f, x, null=("matches", "docids", "rows"))
    assert st == 0
    counts, collapsed = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    hg, hgm = np.full(10, 77, dtype=np.uint32), np.full(10, 77, dtype=np.uint32)
    assert call(hand.qi._h, hand.fd._h, hand.wand._h, 10, terms.ctypes.data, offs.ctypes.data, f._h, x._h, 1, counts.ctypes.data,
                None, collapsed.ctypes.data, scores.ctypes.data, None, hg.ctypes.data, hgm.ctypes.data, None, None, None) == 0
    want = hand.want_c(entry, [[0, 1]], mask, g, 8, 10)
    assert counts[0] == want[0][0] and collapsed[0] == want[4][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))
    assert np.array_equal(hg, want[5][0]) and np.array_equal(hgm, want[6][0])
    x.close()
    f_other.close()
    other.close()
    f.close()


def test_two_threads_one_index_one_facets_handle(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Collapsed(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    g = FA.named_map("clustered", r.num_docs, 300)
    x = r.facets(g, 300)
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    want = {e: r.want_c(e, qs, mask if e == "and" else None, g, 300, 10) for e in ENTRIES}
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine = ENTRIES[which]
            for _ in range(3):
                got = r.run_c(mine, qs, x, f if mine == "and" else None, 10)
                _bit_equal(got[:4] + got[5:], want[mine])
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    f.close()
    x.close()
    r.close()
