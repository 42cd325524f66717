"""Group-limited ranked queries on the GPU through the C ABI (dint_ranked_or_group_limit_queries,
dint_ranked_and_group_limit_queries): counts, BM25 scores, docIDs, matches, kept, skipped,
hit_groups, hit_group_matches and hit_group_ranks equal to the model's (tests/group_limit.py: one lexsort of the model's
matches by (-score, docID), a running count within every group, the cursor on the keys' integers), bit for bit; the facet
rows, matches and blocks_decoded equal to the faceted entry's on the same arguments; per_group = 1 equal to the collapsed
paged entry byte for byte; and the identities with the paged and the filtered entries under the maps that cut no group or
leave one. The index is the hand-made one of the collapse tests: 9 000 documents, a document's lane under list d is d & 63,
norm_lens all 1, so equal scores abound. Every call is made twice and must answer the same bytes. No tolerance anywhere."""
import ctypes as C
import threading

import numpy as np
import pytest

import doc_filter as DF
import facets as FA
import group_limit as GL
import paging as PG
import ranked
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_collapse import hand_maps as collapse_hand_maps
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import BOTH_FORMS, HAND_DOCS
from test_gpu_paging import Paged
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import _hand_made
from test_gpu_ranked_range import HAND_QUERIES
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")
PER_GROUPS = (1, 2, 3, 16)
NONE32 = GL.DEVICE_NONE


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


class Limited(Paged):
    """Paged (an index, its freqs dictionary and wand data on the device, the filtered, faceted, collapsed and paged entries
    and the model's matches) with the two group-limited entries and their model."""

    def run_g(self, entry, qs, facets, n, after, f, k, stats=True, rows=True):
        """-> (counts, scores, docids, matches, blocks_decoded, kept, hit_groups, hit_group_matches, hit_group_ranks, rows,
        skipped); without the stats no matches and blocks_decoded, without the rows no rows"""
        fn = self.qi.ranked_or_group_limit_queries if entry == "or" else self.qi.ranked_and_group_limit_queries
        return fn(self.fd, self.wand, qs, facets, n, after=after, filter=f, k=k, with_stats=stats, with_rows=rows)

    def want_g(self, entry, qs, mask, group_of, n_groups, k, n, after=None):
        after = after if after is not None else [None] * len(qs)
        return GL.stacked([GL.group_limit(self.matches_of(entry, q), mask, group_of, n_groups, k, n, c) for q, c in zip(qs, after)], k, n_groups)

    def check_g(self, entry, qs, group_of, n_groups, n, k=10, after=None, mask=None, f=None, facets=None, what=None, faceted=True):
        """the group-limited call (through the handles given, or ones made and closed here) against the model, bit for bit;
        the same call again: the same bytes; and — faceted — its matches, blocks_decoded and rows against the faceted entry"""
        what = (entry, n_groups, n, k, what)
        own_f, own_x = f is None and mask is not None, facets is None
        if own_f:
            f = self.filter(mask)
        if own_x:
            facets = self.facets(group_of, n_groups)
        got = self.run_g(entry, qs, facets, n, after, f, k)
        _bit_equal(got[:4] + got[5:], self.want_g(entry, qs, mask, group_of, n_groups, k, n, after), what)
        assert np.array_equal(got[0], np.minimum(got[5] - got[10], k)) and (got[5] <= got[3]).all() and (got[10] <= got[5]).all(), what
        assert (got[8] < n).all(), what
        again = self.run_g(entry, qs, facets, n, after, f, k)
        _bit_equal(again[:4] + again[5:], got[:4] + got[5:], what)
        assert again[4] == got[4], what
        if faceted:
            same = self.run_x(entry, qs, facets, f, k)
            _bit_equal((got[3], got[9]), (same[3], same[5]), what)
            assert got[4] == same[4], what
        short = self.run_g(entry, qs, facets, n, after, f, k, stats=False, rows=False)  # (without the stats and the rows: the same)
        assert len(short) == 8, what
        _bit_equal(short, got[:3] + got[5:9] + got[10:], what)
        if own_f:
            f.close()
        if own_x:
            facets.close()
        return got

    def kept_by_group(self, entry, q, group_of, n_groups, n, mask=None):
        """the model's kept documents of a query, per group in key order: {group: [docids]} (NONE32: the ungrouped)"""
        _, ids, groups, _, _ = GL.whole_order(self.matches_of(entry, q), mask, group_of, n_groups, n)
        out = {}
        for d, g in zip(ids.tolist(), groups.tolist()):
            out.setdefault(g, []).append(d)
        return out


@pytest.fixture(scope="module")
def hand(device):
    """test_gpu_ranked_range.py's hand-made index: a = 0 .. 2999, b = 5000 .. 8999 (5000 .. 5006 have freq 3), c = the evens,
    d = every doc (page j holds 256 j .. 256 j + 255: a document's lane is d & 63), e = {10, 20, 30, 40}; norm_lens all 1."""
    kind = host.MULTI_PACKED
    r = Limited(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    yield r
    r.close()


# ---- kernel edges on the hand-made index --------------------------------------------------------------------------------
def limit_map(n_groups, n):
    """The map the limit is about, for per_group n. Under [3] every score is equal and a group's key order is its docID
    order; under [3, 4] the documents 10, 20, 30, 40 score highest; under [2, 3, 4] the evens score above the odds.
      group 1          5 .. 25: one run of one wave; under [3, 4] its best are 10 and 20 (equal), then 5, 6, ... (equal)
      group 2          its n-th match (under [3]) in lane 62, its (n + 1)-th in lane 63 of page 0
      group 3          its n-th match in lane 63, its (n + 1)-th in lane 64 of page 1: the top n ends with its wave
      group 4          its n-th match at page 2's last slot, its (n + 1)-th at page 3's first: the top n from two pages
      groups 5, 6, 7   n - 1, n and n + 1 documents from 1000, 1100 and 1200
      group 0          from 1280 on, 2 n + 2 documents: group 0 in lane 0 of page 5
      the last group   1600 .. 1727 and 2900 .. 5100: two waves and two pages of d, and a's last and b's first pages under [0, 1]
    Everything else is in no group."""
    where = np.full(HAND_DOCS, FA.NONE, dtype=np.int64)
    where[5:26] = 1
    where[63 - n:63 + n + 1] = 2
    where[256 + 64 - n:256 + 64 + n + 1] = 3
    where[768 - n:768 + n + 1] = 4
    where[1000:1000 + n - 1] = 5
    where[1100:1100 + n] = 6
    where[1200:1200 + n + 1] = 7
    where[1280:1280 + 2 * n + 2] = 0
    where[1600:1728] = n_groups - 1
    where[2900:5101] = n_groups - 1
    return where


def all_maps(n_groups, n):
    maps = dict(collapse_hand_maps(n_groups))
    maps["the limit's own"] = limit_map(n_groups, n)
    return maps


MAP_NAMES = list(all_maps(300, 2))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_groups", BOTH_FORMS)
@pytest.mark.parametrize("n", PER_GROUPS)
def test_kernel_edges(hand, entry, n_groups, n):
    """HAND_QUERIES under every hand-made map of the facet and the collapse tests and under the limit's own: among the queries
    [3] (full pages of consecutive documents, every score equal), [3, 4] and [2, 3, 4] (a few documents above the others),
    [0, 1] (a group over the pages of two terms, OR), [0, 2] and [1, 2, 3] (a dead slot between two live ones of a group);
    among the maps a NONE document between two of one group, group 0 in lane 0, the last group, and short maps."""
    for name, g in all_maps(n_groups, n).items():
        x = hand.facets(g, n_groups)
        got = hand.check_g(entry, HAND_QUERIES, g, n_groups, n, k=10, facets=x, what=name)
        for i in (2, 3, 7, 14):  # one query per call: the same answer, a deeper k the same prefix
            one = hand.run_g(entry, [HAND_QUERIES[i]], x, n, None, None, 1000)
            assert one[5][0] == got[5][i] and one[3][0] == got[3][i]
            for j in (1, 2, 6, 7, 8):
                assert np.asarray(one[j][0][:10]).tobytes() == np.asarray(got[j][i]).tobytes(), (name, i, j)
        x.close()


@pytest.mark.parametrize("n", PER_GROUPS)
def test_the_edge_cases_are_what_they_are_said_to_be(hand, n):
    n_groups = 257
    g = limit_map(n_groups, n)
    last = n_groups - 1
    by = hand.kept_by_group("or", [3], g, n_groups, n)
    # a group's top n in one run of a wave; the n-th and the (n + 1)-th match in lanes 62 | 63, 63 | 64 (the run goes on in
    # the next wave) and at a page's last slot (the group goes on in the next page): equal scores straddle the cut, and the
    # smaller docID takes the last place
    assert by[1] == list(range(5, 5 + n)) and 5 + n <= 26
    assert by[2] == list(range(63 - n, 63)) and by[2][-1] & 63 == 62 and g[63] == 2
    assert by[3] == list(range(320 - n, 320)) and by[3][-1] & 63 == 63 and g[320] == 3 and 320 & 63 == 0
    assert by[4] == list(range(768 - n, 768)) and by[4][-1] & 255 == 255 and g[768] == 4
    # exactly n - 1, n and n + 1 matches
    assert by.get(5, []) == list(range(1000, 1000 + n - 1)) and by[6] == list(range(1100, 1100 + n)) and by[7] == list(range(1200, 1200 + n))
    row = FA.row_of(g, n_groups, hand.matches_of("or", [3])[1])[0]
    assert row[5:8].tolist() == [n - 1, n, n + 1]
    # group 0 in lane 0, and the last group from two waves, two pages and — under [0, 1] — the pages of two terms
    assert by[0] == list(range(1280, 1280 + n)) and 1280 & 255 == 0
    assert by[last] == list(range(1600, 1600 + n))
    two_terms = hand.kept_by_group("or", [0, 1], g, n_groups, n)[last]
    sc, ids = hand.matches_of("or", [0, 1])
    assert sc[ids == 2999][0] > sc[ids == 5000][0] > sc[ids == 5007][0]  # a's documents above b's, 5000 .. 5006 above b's others
    assert two_terms == list(range(1600, 1600 + n))  # (a's documents score alike: the smaller docIDs lead)
    two_terms =hand.kept_by_group("or", [0, 1], np.where(g == last, np.where(np.arange(HAND_DOCS) < 2998, FA.NONE, last), g), n_groups, n)[last]
    assert two_terms == [2998, 2999, 5000, 5001, 5002, 5003, 5004, 5005, 5006, 5007, 5008, 5009, 5010, 5011, 5012, 5013][:n]  # both terms' pages
    # equal scores inside the top n, and the higher scores first: under [3, 4] group 1 shows 10 and 20, then 5, 6, ...
    by = hand.kept_by_group("or", [3, 4], g, n_groups, n)
    assert by[1] == ([10, 20] + list(range(5, 10)) + list(range(11, 20)))[:n]
    # under [2, 3, 4] the evens lead: the top n of group 3 comes from two waves of a page as soon as n >= 2
    by = hand.kept_by_group("or", [2, 3, 4], g, n_groups, n)
    evens = [d for d in range(320 - n, 320 + n + 1) if d % 2 == 0]
    odds = [d for d in range(320 - n, 320 + n + 1) if d % 2]
    assert by[3] == (evens + odds)[:n] and (n == 1 or {d >> 6 for d in by[3]} == {4, 5})
    # a dead slot between two live ones of a group: in a's pages the intersection [0, 2] has every other slot dead
    by = hand.kept_by_group("and", [0, 2], g, n_groups, n)
    assert by[4] == [d for d in range(768 - n, 768 + n + 1) if d % 2 == 0][:n]
    # a NONE document between two of one group: it is kept beside the group's n best
    none_between = collapse_hand_maps(n_groups)["a NONE document between two of one group"]
    w = hand.want_g("or", [[3]], None, none_between, n_groups, 40, n)
    ungrouped = w[2][0][:int(w[0][0])][w[5][0][:int(w[0][0])] == NONE32].tolist()
    assert ungrouped == [100, 101, 127, 128, 2999] and w[4][0] == 5 + n


@pytest.mark.parametrize("entry", ENTRIES)
def test_edges_under_a_filter(hand, entry):
    """the filter path: pages are the live blocks, and what they hold outside the filter is dead before a place is taken — a
    group's best outside the filter: the next ones move up; the empty filter: nothing is kept"""
    out = (10, 30, 61, 62, 319, 767, 1100, 1280, 1600, 2900, 2901)
    for members in ([63, 64, 65], list(range(200, 900)) + [2999, 8999], list(range(0, HAND_DOCS, 3)), [d for d in range(HAND_DOCS) if d not in out], []):
        mask = DF.as_mask(members, HAND_DOCS)
        f = hand.filter(mask)
        for n_groups in BOTH_FORMS:
            for n in (2, 3):
                maps = all_maps(n_groups, n)
                for name in ("the limit's own", "a run ends at lane 63, the next begins a wave", "clustered", "every other document NONE",
                             "the map ends inside a page", "one group over the pages of two terms"):
                    got = hand.check_g(entry, HAND_QUERIES, maps[name], n_groups, n, mask=mask, f=f, what=(name, len(members)))
                    assert members or not (got[3].any() or got[5].any() or got[0].any())
        f.close()
    mask = DF.as_mask([d for d in range(HAND_DOCS) if d not in out], HAND_DOCS)
    by = hand.kept_by_group("or", [3, 4], limit_map(257, 2), 257, 2, mask)
    # without 10 group 1 shows 20, then the first of the equal rest; without 61 and 62 group 2 (61 .. 65) shows 63 and 64
    assert by[1] == [20, 5] and by[2] == [63, 64] and by[6] == [1101] and by[0] == [1281, 1282] and by[256] == [1601, 1602]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_groups", BOTH_FORMS)
def test_per_group_of_one_is_the_collapsed_paged_entry(hand, entry, n_groups):
    """byte for byte, with a cursor and without, with a filter and without; every rank is 0"""
    mask = DF.as_mask(list(range(0, HAND_DOCS, 3)), HAND_DOCS)
    f = hand.filter(mask)
    for name in ("the limit's own", "groups of a hundred documents", "clustered", "the map ends inside a page", "one group"):
        g = all_maps(n_groups, 1)[name]
        x = hand.facets(g, n_groups)
        for m, filt in ((None, None), (mask, f)):
            third = [PG.last_hit(*PG.collapsed_page_after(hand.matches_of(entry, q), m, g, n_groups, None, 3)[:3]) for q in HAND_QUERIES]
            for after in (None, third, [(0.0, 0)] * len(HAND_QUERIES), [(np.inf, 7)] * len(HAND_QUERIES)):
                for k in (10, 1000):
                    got = hand.run_g(entry, HAND_QUERIES, x, 1, after, filt, k)
                    same = hand.run_cp(entry, HAND_QUERIES, x, after, filt, k)
                    _bit_equal(got[:4] + got[5:8] + got[9:], same[:4] + same[5:], (entry, name, k))
                    assert got[4] == same[4] and not got[8].any()
        x.close()
    f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_maps_that_cut_no_group_or_leave_one(hand, entry):
    """Map "none", and every document its own group (9 000 groups): the paged entry's answer, bit for bit, kept == matches and
    every rank 0. "One group": the filtered call's top n, ranks 0 .. n - 1, hit_group_matches == matches."""
    mask = DF.as_mask(list(range(0, HAND_DOCS, 3)), HAND_DOCS)
    f = hand.filter(mask)
    for g, n_groups in ((FA.named_map("none", HAND_DOCS, 256), 256), (np.arange(HAND_DOCS, dtype=np.int64), HAND_DOCS)):
        x = hand.facets(g, n_groups)
        for filt, m in ((None, None), (f, mask)):
            after = [PG.last_hit(*PG.page_after(hand.matches_of(entry, q), m, None, 5)[:3]) for q in HAND_QUERIES]
            for n in (1, 3, 16):
                for k, cursors in ((10, None), (1000, after)):
                    got = hand.check_g(entry, HAND_QUERIES, g, n_groups, n, k=k, after=cursors, mask=m, f=filt, facets=x)
                    same = hand.run_p(entry, HAND_QUERIES, cursors, filt, k)
                    _bit_equal(got[:4] + got[10:], same[:4] + same[5:], (entry, n_groups, n, k))
                    assert got[4] == same[4] and np.array_equal(got[5], got[3]) and not got[8].any()
        x.close()
    for n_groups in BOTH_FORMS + (1,):
        g = FA.named_map("one group", HAND_DOCS, n_groups)
        x = hand.facets(g, n_groups)
        for filt, m in ((None, None), (f, mask)):
            for n in PER_GROUPS:
                got = hand.check_g(entry, HAND_QUERIES, g, n_groups, n, k=20, mask=m, f=filt, facets=x)
                top = hand.run_f(entry, HAND_QUERIES, filt, n)
                assert np.array_equal(got[0], np.minimum(got[3], n)) and np.array_equal(got[5], got[0])
                assert got[1][:, :n].tobytes() == top[1].tobytes() and got[2][:, :n].tobytes() == top[2].tobytes()
                for i in range(len(HAND_QUERIES)):
                    c = int(got[0][i])
                    assert got[8][i][:c].tolist() == list(range(c)) and (got[7][i][:c] == got[3][i]).all() and (got[6][i][:c] == n_groups - 1).all()
        x.close()
    f.close()


# ---- call shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest_below_and_above_kept(hand, entry):
    g = np.arange(HAND_DOCS, dtype=np.int64) // 4 % 3000
    x = hand.facets(g, 3000)
    for n in (2, 16):
        for k in (1, 1024):
            got = hand.check_g(entry, HAND_QUERIES, g, 3000, n, k=k, facets=x)
        assert int(got[0].max()) == 1024 and int(got[5].max()) > 1024 and 0 < int(got[5][got[5] > 0].min()) < 1024  # k below and above kept
        assert (n == 2) == (int(got[3].max()) > int(got[5].max()))  # (groups of four documents: 16 a group cuts nothing)
    x.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_batch_of_300_is_one_query_per_call(hand, entry):
    qs = (HAND_QUERIES * 20)[:300]
    g = limit_map(257, 3)
    x = hand.facets(g, 257)
    after = [PG.last_hit(*GL.group_limit(hand.matches_of(entry, q), None, g, 257, 2, 3)[:3]) if i % 3 else None for i, q in enumerate(qs)]
    got = hand.check_g(entry, qs, g, 257, 3, k=10, after=after, facets=x)
    for i in range(0, 300, 7):
        one = hand.run_g(entry, [qs[i]], x, 3, [after[i]], None, 10)
        for j in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10):
            assert np.asarray(one[j][0]).tobytes() == np.asarray(got[j][i]).tobytes(), (entry, i, j)
        assert one[4] <= got[4]
    x.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: a pass holds whole queries, so a query's rounds complete within its
    pass; the table, the counters and the hits of the queries of later passes lie at their own offset, cleared once."""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Limited(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2) + [[], [0]]
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    device.set_option("query_or_pass_pages", pass_pages)
    rng = np.random.default_rng(11)
    for n_groups, name, n in ((8, "clustered", 3), (1000, "striped", 2)):
        g = FA.named_map(name, r.num_docs, n_groups)
        x = r.facets(g, n_groups)
        for entry in ENTRIES:
            after = []
            for q in qs:
                sc, ids = r.ordered(entry, q, None)
                after.append(PG.draw_cursor(rng, sc, ids, r.num_docs) if ids.size else None)
            got = r.check_g(entry, qs, g, n_groups, n, after=after, facets=x, what=name)
            back = r.run_g(entry, qs[::-1], x, n, after[::-1], None, 10)
            for j in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10):
                assert np.asarray(back[j][::-1]).tobytes() == np.asarray(got[j]).tobytes(), (name, entry, j)
            r.check_g(entry, qs, g, n_groups, n, mask=mask, f=f, facets=x, what=(name, "runs"), faceted=False)
        assert int(got[5][len(qs) // 2:].sum()) > 0 and int(got[8].max()) == n - 1  # (queries of later passes keep something)
        x.close()
    f.close()
    r.close()


def _walk(hand, entry, q, g, n_groups, n, k, x, mask=None, f=None):
    sc, ids, groups, group_matches, ranks = GL.whole_order(hand.matches_of(entry, q), mask, g, n_groups, n)
    cur, seen, pages = None, [[], [], [], [], []], 0
    while True:
        got = hand.run_g(entry, [q], x, n, [cur], f, k)
        c = int(got[0][0])
        assert int(got[10][0]) == len(seen[1]) and int(got[5][0]) == ids.size, (entry, q, k, pages)  # skipped: the hits before
        for acc, j in zip(seen, (1, 2, 6, 7, 8)):
            acc += got[j][0][:c].tolist()
        pages += 1
        if c < k:
            assert int(got[10][0]) + c == ids.size  # the final page is short
            break
        cur = PG.last_hit(c, got[1][0], got[2][0])
    assert seen[1] == ids.tolist() and np.array(seen[0], dtype=np.float32).tobytes() == sc.tobytes(), (entry, q, k)
    assert seen[2] == groups.tolist() and seen[3] == group_matches.tolist() and seen[4] == ranks.tolist()
    return pages


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_walk_reproduces_the_whole_kept_order(hand, entry):
    """pages of 7 chained by the last hit, and the same through ranked_pages: "more results, at most n per site" """
    mask = DF.as_mask(list(range(0, HAND_DOCS, 3)), HAND_DOCS)
    f = hand.filter(mask)
    for n_groups, n in ((256, 2), (257, 3)):
        g = collapse_hand_maps(n_groups)["groups of a hundred documents"]
        x = hand.facets(g, n_groups)
        q = [3] if entry == "or" else [0, 2]
        assert _walk(hand, entry, q, g, n_groups, n, 7, x) > 8
        assert _walk(hand, entry, q, g, n_groups, n, 7, x, mask, f) > 8
        qs = [q, [2, 3, 4], [4], []]
        seen = {i: [] for i in range(len(qs))}
        before = {i: 0 for i in range(len(qs))}
        for ids, counts, scores, docids, skipped in hand.qi.ranked_pages(f"{entry}_group_limit", hand.fd, hand.wand, qs, k=7, facets=x, per_group=n):
            for j, i in enumerate(ids.tolist()):
                assert int(skipped[j]) == before[i]
                seen[i] += docids[j][:int(counts[j])].tolist()
                before[i] += int(counts[j])
        for i, qq in enumerate(qs):
            assert seen[i] == GL.whole_order(hand.matches_of(entry, qq), None, g, n_groups, n)[1].tolist(), (entry, qq)
        assert len(list(hand.qi.ranked_pages(f"{entry}_group_limit", hand.fd, hand.wand, qs, k=7, facets=x, per_group=n, max_pages=1))) == 1
        x.close()
    f.close()


def test_calls_in_a_row_leave_nothing_stale(hand):
    """one index, different batches and per_groups, collapsed and group-limited calls in turn (they share the slots' groups):
    a longer batch first, then shorter ones, other group counts in between — a key, a counter or a hit that a later call did
    not clear would show. Two queries of a batch that hit the same groups keep their own tables; an empty query inside."""
    g8, g300 = FA.named_map("striped", HAND_DOCS, 8), FA.named_map("clustered", HAND_DOCS, 300)
    x8, x300 = hand.facets(g8, 8), hand.facets(g300, 300)
    for entry in ENTRIES:
        hand.check_g(entry, HAND_QUERIES, g8, 8, 16, facets=x8)
        hand.check_c(entry, HAND_QUERIES, g8, 8, facets=x8)
        hand.check_g(entry, [[4], [], [0, 1]], g8, 8, 2, facets=x8)
        hand.check_g(entry, HAND_QUERIES[::-1], g300, 300, 3, facets=x300)
        hand.check_c(entry, [[3], [3, 4]], g300, 300, facets=x300)
        hand.check_g(entry, [[], []], g300, 300, 16, facets=x300)
        got = hand.check_g(entry, [[4]], g8, 8, 1, facets=x8)
        assert got[2][0][:4].tolist() == [10, 20, 30, 40] and got[6][0][:5].tolist() == [2, 4, 6, 0, NONE32] and got[5][0] == 4
        got = hand.check_g(entry, [[3], [3, 4], [], [3], [2, 3, 4]], g300, 300, 2, k=700, facets=x300)
        assert got[5].tolist()[:4] == ([600, 600, 0, 600] if entry == "or" else [600, 4, 0, 600])
        assert not got[0][2] and (got[6][2] == NONE32).all() and not got[7][2].any() and not got[8][2].any()
    x8.close()
    x300.close()


# ---- docIDs at the top of the u32 range ---------------------------------------------------------------------------------
def test_docids_near_2_to_the_32(device):
    """An index with docIDs up to 0xFFFFFFFE: the key's low word is the inverted docID, 1 for the largest one, and a map that
    ends far below leaves every high document in no group — the map is never read past its end."""
    kind = host.SINGLE_PACKED
    lists = [np.arange(TOP - 599, TOP + 1, dtype=np.uint64).astype(np.uint32), np.array([0, 5, TOP], dtype=np.uint32),
             np.concatenate([np.arange(0, 300, 3, dtype=np.uint64), np.arange(TOP - 298, TOP + 1, 2, dtype=np.uint64)]).astype(np.uint32),
             np.arange((1 << 31) - 300, (1 << 31) + 300, dtype=np.uint64).astype(np.uint32)]
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 3, x.size).astype(np.uint32) for x in lists]
    h = HighIndex(device, kind, lists, freqs)
    num_docs = TOP + 1
    nl = np.zeros(num_docs, dtype=np.float32)  # (pages of zeros the host never touches but where a posting lies)
    nl[h.docids] = 1.0  # (equal scores among the high documents)
    qi, wand = device.QueryIndex(h.dd, h.index, h.offsets), device.WandData(nl)
    bl = ranked.BuilderLists(h.docids, h.freqs, h.bounds)
    qs = [[0], [1], [0, 1], [0, 2], [1, 2], [0, 1, 2], [2, 2, 1], [3], [0, 3], [1, 3], []]
    every = {conj: [GL.every_match(bl, q, nl, num_docs, conj) for q in qs] for conj in (False, True)}
    for n_map, n_groups, name, n in ((100, 7, "striped", 2), (6, 300, "striped", 16), (1000, 256, "clustered", 3), (1, 1, "one group", 1)):
        g = FA.named_map(name, n_map, n_groups)
        x = device.DocFacets(0, g, n_groups)
        for entry in ENTRIES:
            fn = qi.ranked_or_group_limit_queries if entry == "or" else qi.ranked_and_group_limit_queries
            after = []
            for m in every[entry == "and"]:
                sc, ids = PG.in_filter(m, None)
                after.append((sc[min(1, ids.size - 1)], int(ids[min(1, ids.size - 1)])) if ids.size else None)
            after[0] = (after[0][0], 0xFFFFFFFF)  # past every docID of its score
            for cursors in (None, after):
                got = fn(h.fd, wand, qs, x, n, after=cursors, k=10, with_stats=True, with_rows=True)
                want = GL.stacked([GL.group_limit(e, None, g, n_groups, 10, n, c) for e, c in zip(every[entry == "and"], cursors or [None] * len(qs))],
                                  10, n_groups)
                _bit_equal(got[:4] + got[5:], want, (n_map, entry))
            assert (got[5].astype(np.int64) >= [int((e[1] >= n_map).sum()) for e in every[entry == "and"]]).all()
        x.close()
    qi.close()
    wand.close()


# ---- errors, and two threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, entry):
    call = getattr(device._lib, f"dint_ranked_{entry}_group_limit_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    g = FA.named_map("striped", HAND_DOCS, 8)
    x = hand.facets(g, 8)
    good = np.array([(1.0, 3)], dtype=device._CURSOR)
    nan = np.array([(np.nan, 3)], dtype=device._CURSOR)

    def attempt(k, terms_, filt, fac, n_per=2, cursor=good, null=(), offs_=offs, n=1):
        """null: the outputs passed as null pointers -> (status, every output still holds its canary)"""
        out = {"counts": np.full(1, 77, dtype=np.uint64), "matches": np.full(1, 77, dtype=np.uint64), "kept": np.full(1, 77, dtype=np.uint64),
               "skipped": np.full(1, 77, dtype=np.uint64), "scores": np.full(1025, -1.0, dtype=np.float32),
               "docids": np.full(1025, 77, dtype=np.uint32), "hit_groups": np.full(1025, 77, dtype=np.uint32),
               "hit_group_matches": np.full(1025, 77, dtype=np.uint32), "hit_group_ranks": np.full(1025, 77, dtype=np.uint32),
               "rows": np.full(16, 77, dtype=np.uint32)}
        blocks = C.c_uint64(77)
        p = {name: None if name in null else a.ctypes.data for name, a in out.items()}
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  fac._h if fac is not None else None, n_per, cursor.ctypes.data if cursor is not None else None, n, p["counts"], p["matches"],
                  p["kept"], p["skipped"], p["scores"], p["docids"], p["hit_groups"], p["hit_group_matches"], p["hit_group_ranks"], p["rows"],
                  C.byref(blocks), None)
        untouched = all((a == (-1.0 if name == "scores" else 77)).all() for name, a in out.items()) and blocks.value == 77
        return st, untouched, out

    for filt in (None, f):
        assert attempt(0, terms, filt, x)[:2] == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, x)[:2] == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 5], dtype=np.uint32), filt, x)[:2] == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, x, offs_=np.array([2, 0], dtype=np.uint64))[:2] == (DINT_ERR_ARG, True)  # decreasing offsets
        assert attempt(10, terms, filt, None)[:2] == (DINT_ERR_ARG, True)  # no facets
        assert attempt(10, terms, filt, x, cursor=nan)[:2] == (DINT_ERR_ARG, True)
        for n_per in (0, 17):
            assert attempt(10, terms, filt, x, n_per=n_per)[:2] == (DINT_ERR_ARG, True)
        for name in ("counts", "scores", "kept", "hit_groups", "hit_group_matches", "hit_group_ranks"):
            assert attempt(10, terms, filt, x, null=(name,))[:2] == (DINT_ERR_ARG, True), name
    assert attempt(10, terms, f_other, x)[:2] == (DINT_ERR_ARG, True)  # a filter of another query index
    # n_queries * n_groups * per_group past 2^27: refused before the offsets are read (2^27 itself is not refused for its size)
    big = hand.facets(np.zeros(1, dtype=np.int64), 65536)
    for n_per, n in ((1, (1 << 11) + 1), (2, (1 << 10) + 1), (16, (1 << 7) + 1)):
        assert attempt(10, terms, None, big, n_per=n_per, n=n, cursor=None)[:2] == (DINT_ERR_ARG, True)
    big.close()
    st, untouched, _ = attempt(10, terms, f, x)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_g(entry, [[5]], x, 2, None, f, 10)
    with pytest.raises(device.DintError):
        hand.run_g(entry, [[0]], x, 2, None, f_other, 10)
    with pytest.raises(device.DintError):
        hand.run_g(entry, [[0, 1]], x, 2, [(float("nan"), 0)], None, 10)
    with pytest.raises(ValueError):
        hand.run_g(entry, [[0, 1]], x, 17, None, None, 10)
    # the nullable outputs — matches, skipped, docids, facet_counts, blocks_decoded, the cursors and the filter — change nothing else
    want = hand.want_g(entry, [[0, 1]], mask, g, 8, 10, 2, [(1.0, 3)])
    for null, cursor in ((("matches", "skipped", "docids", "rows"), good), ((), good)):
        st, _, out = attempt(10, terms, f, x, null=null, cursor=cursor)
        assert st == 0 and out["counts"][0] == want[0][0] and out["kept"][0] == want[4][0]
        assert out["scores"][:10].tobytes() == want[1][0].tobytes() and np.array_equal(out["hit_groups"][:10], want[5][0])
        assert np.array_equal(out["hit_group_matches"][:10], want[6][0]) and np.array_equal(out["hit_group_ranks"][:10], want[7][0])
        assert "skipped" in null or out["skipped"][0] == want[9][0]
    assert attempt(10, terms, None, x, cursor=None)[0] == 0
    x.close()
    f_other.close()
    other.close()
    f.close()


def test_two_threads_one_index_one_facets_handle(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Limited(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    g = FA.named_map("clustered", r.num_docs, 300)
    x = r.facets(g, 300)
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    per = {"or": 2, "and": 16}
    want = {e: r.want_g(e, qs, mask if e == "and" else None, g, 300, 10, per[e]) for e in ENTRIES}
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine = ENTRIES[which]
            for _ in range(3):
                got = r.run_g(mine, qs, x, per[mine], None, f if mine == "and" else None, 10)
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
