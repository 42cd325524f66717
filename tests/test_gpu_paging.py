"""search_after paging of the ranked queries on the GPU through the C ABI (dint_ranked_or_paged_queries,
dint_ranked_and_paged_queries and the two collapsed paged entries): counts, BM25 scores, docIDs, matches
and skipped equal to the model's (tests/paging.py: the matches in key order, cut strictly behind the cursor), bit for bit;
matches and blocks_decoded equal to the filtered entry's; a from-the-start call equal to the filtered entry's answer. The
index is the hand-made one of the range and collapse tests: 9 000 documents, a document's lane is d & 63, norm_lens all 1, so
equal scores abound. No tolerance anywhere."""
import ctypes as C
import threading

import numpy as np
import pytest

import doc_filter as DF
import facets as FA
import paging as PG
import ranked
import ranked_range as RR
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_collapse import Collapsed
from test_gpu_collapse import hand_maps as collapse_hand_maps
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import BOTH_FORMS, HAND_DOCS
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import _hand_made
from test_gpu_ranked_range import HAND_QUERIES
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")


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


class Paged(Collapsed):
    """Collapsed (an index, its freqs dictionary and wand data on the device, the filtered and collapsed entries and the
    model's matches) with the four paged entries and their model."""

    def run_p(self, entry, qs, after, f, k, stats=True):
        """-> (counts, scores, docids, matches, blocks_decoded, skipped); without the stats no matches and blocks_decoded"""
        fn = self.qi.ranked_or_paged_queries if entry == "or" else self.qi.ranked_and_paged_queries
        return fn(self.fd, self.wand, qs, after=after, filter=f, k=k, with_stats=stats)

    def want_p(self, entry, qs, after, mask, k):
        after = after if after is not None else [None] * len(qs)
        return PG.stacked([PG.page_after(self.matches_of(entry, q), mask, c, k) for q, c in zip(qs, after)], k)

    def check_p(self, entry, qs, after, k=10, mask=None, f=None, what=None):
        """the paged call against the model, bit for bit, and its matches and blocks_decoded against the filtered entry"""
        what = (entry, k, what)
        own_f = f is None and mask is not None
        if own_f:
            f = self.filter(mask)
        got = self.run_p(entry, qs, after, f, k)
        _bit_equal(got[:4] + got[5:], self.want_p(entry, qs, after, mask, k), what)
        assert np.array_equal(got[0], np.minimum(got[3] - got[5], k)), what
        same = self.run_f(entry, qs, f, k)
        _bit_equal((got[3],), (same[3],), what)
        assert got[4] == same[4], what
        short = self.run_p(entry, qs, after, f, k, stats=False)
        assert len(short) == 4, what
        _bit_equal(short, got[:3] + got[5:], what)
        if own_f:
            f.close()
        return got

    def run_cp(self, entry, qs, facets, after, f, k):
        """-> (counts, scores, docids, matches, blocks_decoded, collapsed, hit_groups, hit_group_matches, rows, skipped)"""
        fn = self.qi.ranked_or_collapsed_paged_queries if entry == "or" else self.qi.ranked_and_collapsed_paged_queries
        return fn(self.fd, self.wand, qs, facets, after=after, filter=f, k=k, with_stats=True, with_rows=True)

    def ordered(self, entry, q, mask=None):
        """the query's matches under the mask in key order: (scores, docids)"""
        return PG.in_filter(self.matches_of(entry, q), mask)


@pytest.fixture(scope="module")
def hand(device):
    """test_gpu_ranked_range.py's hand-made index: a = 0 .. 2999, b = 5000 .. 8999 (5000 .. 5006 have freq 3), c = the evens,
    d = every doc (page j holds 256 j .. 256 j + 255: a document's lane is d & 63), e = {10, 20, 30, 40}; norm_lens all 1."""
    kind = host.MULTI_PACKED
    r = Paged(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    yield r
    r.close()


CLUSTERED = DF.as_mask(list(range(200, 600)) + list(range(2900, 5300)) + [8999], HAND_DOCS)  # dead blocks between live ones


def _filters(hand):
    return ((None, None), (CLUSTERED, hand.filter(CLUSTERED)))


# ---- cursor edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_cursor_edges(hand, entry):
    for mask, f in _filters(hand):
        firsts = [hand.ordered(entry, q, mask) for q in HAND_QUERIES]
        at = lambda i: [((sc[i], int(ids[i])) if ids.size else None) for sc, ids in firsts]  # noqa: E731
        got = hand.check_p(entry, HAND_QUERIES, at(0), mask=mask, f=f, what="the first match")
        assert np.array_equal(got[5], (got[3] > 0).astype(np.uint64))
        got = hand.check_p(entry, HAND_QUERIES, at(-1), mask=mask, f=f, what="the last match")
        assert not got[0].any() and np.array_equal(got[5], got[3]) and got[3].sum() > 1000
        same = hand.run_f(entry, HAND_QUERIES, f, 10)
        for after in (None, [None] * len(HAND_QUERIES), [(np.inf, 5)] * len(HAND_QUERIES)):
            got = hand.check_p(entry, HAND_QUERIES, after, mask=mask, f=f, what="from the start")
            _bit_equal(got[:4], same[:4], entry)
            assert not got[5].any() and got[4] == same[4]
        for s in (0.0, -0.0, 1e-45, np.float32(1e-39), -1.0, -np.inf):  # 1e-45 and 1e-39: subnormals, below every score
            got = hand.check_p(entry, HAND_QUERIES, [(s, 0)] * len(HAND_QUERIES), mask=mask, f=f, what=("nothing after", s))
            assert not got[0].any() and np.array_equal(got[5], got[3]) and not got[1].any() and (got[2] == 0xFFFFFFFF).all()
        if f is not None:
            f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_ties_across_the_cursor_and_bits_without_tolerance(hand, entry):
    """[3] scores every document the same; [2, 3] the evens above the odds (OR) or the evens alike (AND); [0, 1] (OR) a's
    documents above b's. The cursor inside a run of equal scores: a match, a docID that is no match between two matched ones
    (under the filter, and an odd docID in c's AND), docID 0 and docID 0xFFFFFFFF; then the floats next to a match's score."""
    for mask, f in _filters(hand):
        for q in ([3], [2, 3], [0, 1], [3, 4]):
            sc, ids = hand.ordered(entry, q, mask)
            if ids.size < 3:
                continue
            s = sc[ids.size // 2]
            run = ids[sc == s]  # (ascending: the key order of equal scores)
            if run.size < 3:
                continue
            inside = int(run[run.size // 2])
            assert run[0] < inside < run[-1]  # matches of that score on both sides
            gaps = np.flatnonzero(np.diff(run.astype(np.int64)) > 1)
            cursors = [(s, inside), (s, 0), (s, 0xFFFFFFFF), (s, int(run[0])), (s, int(run[-1]))]
            if gaps.size:
                cursors.append((s, int(run[gaps[0]]) + 1))  # no match, between two matched docIDs
            top = np.float32(np.inf)
            cursors += [(np.nextafter(s, top), 0), (np.nextafter(s, top), 0xFFFFFFFF), (np.nextafter(s, np.float32(0)), 0),
                        (np.nextafter(s, np.float32(0)), 0xFFFFFFFF)]
            assert not np.isin([np.nextafter(s, top), np.nextafter(s, np.float32(0))], sc).any()  # neither equals a match's score
            for k in (10, 300):
                got = hand.check_p(entry, [q] * len(cursors), cursors, k=k, mask=mask, f=f, what=q)
            above, below = int((sc > s).sum()), int((sc >= s).sum())
            assert got[5][1] == above + (1 if run[0] == 0 else 0) and got[5][2] == below
            assert got[5][-4] == got[5][-3] == above and got[5][-2] == got[5][-1] == below
        if f is not None:
            f.close()


def _cut_cases(hand):
    """cursors whose cut falls where the kernel's waves and pages meet, chosen from the model: under [3] (d: page j holds
    256 j .. 256 j + 255, every score equal, key order = docID order) the cut after docID d lies between the slots d and
    d + 1; under OR [0, 1] a's documents all score above b's, so the cursor at a's last document cuts between the pages of two
    terms."""
    sc, ids = hand.ordered("or", [3])
    s = sc[0]
    cases = {"lanes 62 | 63": ([3], (s, 256 + 62)), "lanes 63 | 64": ([3], (s, 256 + 63)), "a page's last slot | the next page's first": ([3], (s, 511)),
             "the index's last page, its last slot": ([3], (s, 8999)), "lane 0 | 1 of the first page": ([3], (s, 0))}
    sc01, ids01 = hand.ordered("or", [0, 1])
    cases["between the pages of two terms"] = ([0, 1], (sc01[ids01 == 2999][0], 2999))
    return cases


def test_the_cut_cases_are_what_they_are_said_to_be(hand):
    sc, ids = hand.ordered("or", [3])
    assert np.unique(sc).size == 1 and np.array_equal(ids, np.arange(HAND_DOCS))  # slot i of page j: document 256 j + i
    cases = _cut_cases(hand)
    for name, d in (("lanes 62 | 63", 318), ("lanes 63 | 64", 319), ("a page's last slot | the next page's first", 511)):
        n, _, docids, m, skipped = PG.page_after(hand.matches_of("or", [3]), None, cases[name][1], 2)
        assert skipped == d + 1 and docids.tolist() == [d + 1, d + 2] and m == 9000
    assert (318 & 63, 319 & 63, 320 & 63, 511 & 255, 512 & 255) == (62, 63, 0, 255, 0)
    sc01, ids01 = hand.ordered("or", [0, 1])
    assert sc01[ids01 < 3000].min() > sc01[ids01 >= 5000].max()  # a is the rarer list: every a above every b
    n, _, docids, m, skipped = PG.page_after(hand.matches_of("or", [0, 1]), None, cases["between the pages of two terms"][1], 3)
    assert skipped == 3000 and docids.tolist() == [5000, 5001, 5002] and m == 7000


@pytest.mark.parametrize("entry", ENTRIES)
def test_cuts_at_slot_boundaries(hand, entry):
    cases = _cut_cases(hand)
    qs, after = [q for q, _ in cases.values()], [c for _, c in cases.values()]
    for k in (1, 2, 300):
        hand.check_p(entry, qs, after, k=k, what="cuts")
    for q, c in zip(qs, after):  # ... and a query per call
        hand.check_p(entry, [q], [c], k=5, what=c)


# ---- the walk -----------------------------------------------------------------------------------------------------------
def _walk(hand, entry, q, k, mask=None, f=None):
    sc, ids = hand.ordered(entry, q, mask)
    cur, seen_sc, seen_ids, pages = None, [], [], 0
    while True:
        got = hand.run_p(entry, [q], [cur], f, k)
        n = int(got[0][0])
        assert int(got[5][0]) == len(seen_ids) and int(got[3][0]) == ids.size, (entry, q, k, pages)  # skipped: the hits before
        seen_sc.append(got[1][0][:n])
        seen_ids += got[2][0][:n].tolist()
        pages += 1
        if n < k:
            assert int(got[5][0]) + n == ids.size  # the final page is short
            break
        cur = PG.last_hit(n, got[1][0], got[2][0])
    assert seen_ids == ids.tolist() and np.concatenate(seen_sc).tobytes() == sc.tobytes(), (entry, q, k)
    return pages


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_walk_reproduces_the_whole_order(hand, entry):
    """queries with more than 1024 matches, chosen from the model; pages of 7 on the smallest of them (a launch per page)"""
    deep = [q for q in HAND_QUERIES if hand.ordered(entry, q)[1].size > 1024]
    assert len(deep) >= 3
    smallest = min(deep, key=lambda q: hand.ordered(entry, q)[1].size)
    largest = max(deep, key=lambda q: hand.ordered(entry, q)[1].size)
    assert _walk(hand, entry, largest, 1024) >= 2
    assert _walk(hand, entry, smallest, 64) > 16
    f = hand.filter(CLUSTERED)
    few = min((q for q in HAND_QUERIES if hand.ordered(entry, q, CLUSTERED)[1].size > 100), key=lambda q: hand.ordered(entry, q, CLUSTERED)[1].size)
    assert _walk(hand, entry, few, 7, CLUSTERED, f) > 14
    assert _walk(hand, entry, largest, 1024, CLUSTERED, f) >= 2
    f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_the_walk_through_ranked_pages(hand, entry):
    qs = [q for q in HAND_QUERIES if hand.ordered(entry, q)[1].size > 1024][:3] + [[4], []]
    k = 1024
    seen = {i: [] for i in range(len(qs))}
    before = {i: 0 for i in range(len(qs))}
    n_pages = 0
    for ids, counts, scores, docids, skipped in hand.qi.ranked_pages(entry, hand.fd, hand.wand, qs, k=k):
        n_pages += 1
        for j, i in enumerate(ids.tolist()):
            assert int(skipped[j]) == before[i]
            seen[i] += docids[j][:int(counts[j])].tolist()
            before[i] += int(counts[j])
    assert n_pages >= 2
    for i, q in enumerate(qs):
        assert seen[i] == hand.ordered(entry, q)[1].tolist(), (entry, q)
    assert len(list(hand.qi.ranked_pages(entry, hand.fd, hand.wand, qs, k=k, max_pages=1))) == 1


# ---- sharding, batches, passes, calls in a row, k -----------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_per_shard_pages_merge_to_the_global_page(hand, entry):
    """interval filters that tile the docID space, one call each under the same cursors: the merge of the parts is the
    unfiltered page"""
    qs = HAND_QUERIES
    after = [PG.last_hit(*PG.page_after(hand.matches_of(entry, q), None, None, 25)[:3]) for q in qs]  # page 2 of 25 a page
    whole = hand.check_p(entry, qs, after, k=25, what="whole")
    parts = []
    for lo, hi in RR.slices(0, HAND_DOCS, 3):
        mask = DF.as_mask(list(range(lo, hi)), HAND_DOCS)
        parts.append(hand.check_p(entry, qs, after, k=25, mask=mask, what=(lo, hi)))
    for i in range(len(qs)):
        merged = RR.merge_topk([(p[0][i], p[1][i], p[2][i]) for p in parts], 25)
        assert merged[0] == whole[0][i] and merged[1].tobytes() == whole[1][i].tobytes() and merged[2].tobytes() == whole[2][i].tobytes()
        assert sum(int(p[5][i]) for p in parts) == int(whole[5][i]) and sum(int(p[3][i]) for p in parts) == int(whole[3][i])


@pytest.mark.parametrize("pass_pages", [0, 1, 2, 7])
def test_a_batch_of_cursors_in_many_passes(device, small_corpus, pass_pages):
    """a different cursor per query and some None, an empty query inside the batch, two queries with equal terms and different
    cursors; query_or_pass_pages cuts the OR call into passes (0: the default), and a later pass's counters lie at the pass's
    query offset"""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Paged(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:60] + heavy_queries(ix.lens, 12, seed=2) + [[], [0]]
    qs = qs + [qs[-3], qs[0]]  # equal terms, other cursors
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    if pass_pages:
        device.set_option("query_or_pass_pages", pass_pages)
    rng = np.random.default_rng(7)
    for entry in ENTRIES:
        for m, filt in ((None, None), (mask, f)):
            after = []
            for q in qs:
                sc, ids = r.ordered(entry, q, m)
                after.append(PG.draw_cursor(rng, sc, ids, r.num_docs) if ids.size else None)
            got = r.check_p(entry, qs, after, mask=m, f=filt, what=pass_pages)
            assert int(got[5][len(qs) // 2:].sum()) > 0 and got[5][-4] == 0 and got[3][-4] == 0
            back = r.run_p(entry, qs[::-1], after[::-1], filt, 10)
            for j in (0, 1, 2, 3, 5):
                assert np.asarray(back[j][::-1]).tobytes() == np.asarray(got[j]).tobytes(), (entry, j)
            # a paged call, then an un-paged one: no stale key or counter
            same = r.run_f(entry, qs, filt, 10)
            start = r.run_p(entry, qs, None, filt, 10)
            _bit_equal(start[:4], same[:4], entry)
            assert not start[5].any()
            r.check_p(entry, qs[:5], after[5:10], mask=m, f=filt, what="a shorter batch behind a longer one")
    f.close()
    r.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, entry):
    after = [PG.last_hit(*PG.page_after(hand.matches_of(entry, q), None, None, 3)[:3]) for q in HAND_QUERIES]
    for k in (1, 1024):
        got = hand.check_p(entry, HAND_QUERIES, after, k=k)
    assert int(got[0].max()) == 1024 and int((got[3] - got[5]).max()) > 1024


# ---- docIDs at the top of the u32 range ---------------------------------------------------------------------------------
def test_docids_near_2_to_the_32(device):
    kind = host.SINGLE_PACKED
    lists = [np.arange(TOP - 599, TOP + 1, dtype=np.uint64).astype(np.uint32), np.array([0, 5, TOP], dtype=np.uint32),
             np.concatenate([np.arange(0, 300, 3, dtype=np.uint64), np.arange(TOP - 298, TOP + 1, 2, dtype=np.uint64)]).astype(np.uint32)]
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 3, x.size).astype(np.uint32) for x in lists]
    h = HighIndex(device, kind, lists, freqs)
    num_docs = TOP + 1
    nl = np.zeros(num_docs, dtype=np.float32)
    nl[h.docids] = 1.0  # (equal scores among the high documents)
    qi, wand = device.QueryIndex(h.dd, h.index, h.offsets), device.WandData(nl)
    bl = ranked.BuilderLists(h.docids, h.freqs, h.bounds)
    qs = [[0], [1], [0, 1], [0, 2], [1, 2], [0, 1, 2], []]
    for entry, fn in (("or", qi.ranked_or_paged_queries), ("and", qi.ranked_and_paged_queries)):
        every = [PG.CO.every_match(bl, q, nl, num_docs, entry == "and") for q in qs]
        for pick in (0, -1, 1):
            after = []
            for m in every:
                sc, ids = PG.in_filter(m, None)
                after.append((sc[min(pick, ids.size - 1)], int(ids[min(pick, ids.size - 1)])) if ids.size else None)
            after[0] = (after[0][0], TOP) if pick == 0 else (after[0][0], 0xFFFFFFFF)  # the largest docID; past every docID
            got = fn(h.fd, wand, qs, after=after, k=10, with_stats=True)
            _bit_equal(got[:4] + got[5:], PG.stacked([PG.page_after(m, None, c, 10) for m, c in zip(every, after)], 10), (entry, pick))
    qi.close()
    wand.close()


# ---- errors, and two threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, entry):
    lib = device._lib
    plain, coll = getattr(lib, f"dint_ranked_{entry}_paged_queries"), getattr(lib, f"dint_ranked_{entry}_collapsed_paged_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    x = hand.facets(FA.named_map("striped", HAND_DOCS, 8), 8)
    good = np.array([(1.0, 3)], dtype=device._CURSOR)
    nan = np.array([(np.nan, 3)], dtype=device._CURSOR)

    def attempt(collapsed, k, terms_, filt, cursor, null=(), offs_=offs, fac=x):
        out = {"counts": np.full(1, 77, dtype=np.uint64), "matches": np.full(1, 77, dtype=np.uint64), "collapsed": np.full(1, 77, dtype=np.uint64),
               "skipped": np.full(1, 77, dtype=np.uint64), "scores": np.full(1025, -1.0, dtype=np.float32),
               "docids": np.full(1025, 77, dtype=np.uint32), "hit_groups": np.full(1025, 77, dtype=np.uint32),
               "hit_group_matches": np.full(1025, 77, dtype=np.uint32), "rows": np.full(16, 77, dtype=np.uint32)}
        blocks = C.c_uint64(77)
        p = {name: None if name in null else a.ctypes.data for name, a in out.items()}
        fp, cp = filt._h if filt is not None else None, cursor.ctypes.data if cursor is not None else None
        if collapsed:
            st = coll(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, fp, fac._h if fac is not None else None,
                      cp, 1, p["counts"], p["matches"], p["collapsed"], p["skipped"], p["scores"], p["docids"], p["hit_groups"],
                      p["hit_group_matches"], p["rows"], C.byref(blocks), None)
        else:
            st = plain(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, fp, cp, 1, p["counts"], p["matches"],
                       p["skipped"], p["scores"], p["docids"], C.byref(blocks), None)
        untouched = all((a == (-1.0 if name == "scores" else 77)).all() for name, a in out.items()) and blocks.value == 77
        return st, untouched

    for collapsed in (False, True):
        for filt in (None, f):
            assert attempt(collapsed, 10, terms, filt, nan) == (DINT_ERR_ARG, True)  # a NaN cursor
            assert attempt(collapsed, 0, terms, filt, good) == (DINT_ERR_ARG, True)
            assert attempt(collapsed, 1025, terms, filt, good) == (DINT_ERR_ARG, True)
            assert attempt(collapsed, 10, np.array([0, 5], dtype=np.uint32), filt, good) == (DINT_ERR_ARG, True)  # a term >= n_lists
            assert attempt(collapsed, 10, terms, filt, good, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)
            for name in ("counts", "scores") + (("collapsed", "hit_groups", "hit_group_matches") if collapsed else ()):
                assert attempt(collapsed, 10, terms, filt, good, null=(name,)) == (DINT_ERR_ARG, True), name
        assert attempt(collapsed, 10, terms, f_other, good) == (DINT_ERR_ARG, True)  # a filter of another query index
        st, untouched = attempt(collapsed, 10, terms, f, good)
        assert st == 0 and not untouched
        assert attempt(collapsed, 10, terms, f, good, null=("matches", "docids", "skipped", "rows"))[0] == 0  # the nullable outputs
        assert attempt(collapsed, 10, terms, f, None)[0] == 0
    assert attempt(True, 10, terms, f, good, fac=None) == (DINT_ERR_ARG, True)  # no facets
    with pytest.raises(device.DintError):
        hand.run_p(entry, [[0, 1]], [(float("nan"), 0)], None, 10)
    x.close()
    f_other.close()
    other.close()
    f.close()


def test_two_threads_one_index(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Paged(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    masks = {"or": None, "and": mask}
    after = {e: [PG.last_hit(*PG.page_after(r.matches_of(e, q), masks[e], None, 4)[:3]) for q in qs] for e in ENTRIES}
    want = {e: r.want_p(e, qs, after[e], masks[e], 10) for e in ENTRIES}
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine = ENTRIES[which]
            for _ in range(3):
                got = r.run_p(mine, qs, after[mine], f if mine == "and" else None, 10)
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
    r.close()


# ---- the collapsed paged entries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_groups", BOTH_FORMS)
def test_the_collapsed_walk(hand, entry, n_groups):
    """On the collapse tests' maps: the walk over the kept documents reproduces the collapsed model's whole order, skipped +
    count reaches collapsed, hit_groups / hit_group_matches come from the model on every page, and matches, collapsed, the
    rows and blocks_decoded are the collapsed entry's on every page."""
    maps = collapse_hand_maps(n_groups)
    qs = [[3], [3, 4], [2, 3, 4], [0, 1], [0, 2], []]
    for name in ("groups of a hundred documents", "the best in the first, a middle and the last lane of its run", "clustered"):
        g = maps[name]
        x = hand.facets(g, n_groups)
        k = 40
        base = hand.run_c(entry, qs, x, None, k)
        cursors, done, seen, pages = [None] * len(qs), [False] * len(qs), [[] for _ in qs], 0
        while not all(done) and pages < 12:
            got = hand.run_cp(entry, qs, x, cursors, None, k)
            want = PG.collapsed_stacked([PG.collapsed_page_after(hand.matches_of(entry, q), None, g, n_groups, c, k)
                                         for q, c in zip(qs, cursors)], k, n_groups)
            _bit_equal(got[:4] + got[5:], want, (entry, name, pages))
            _bit_equal((got[3], got[5], got[8]), (base[3], base[5], base[8]), (entry, name, pages))
            assert got[4] == base[4]
            for i in range(len(qs)):
                n = int(got[0][i])
                assert int(got[9][i]) == len(seen[i]) or done[i]
                if not done[i]:
                    seen[i] += got[2][i][:n].tolist()
                    done[i] = n < k
                    if done[i]:
                        assert int(got[9][i]) + n == int(got[5][i])  # skipped + count reaches collapsed
                    else:
                        cursors[i] = PG.last_hit(n, got[1][i], got[2][i])
            pages += 1
        for i, q in enumerate(qs):
            whole = PG.CO.collapse(hand.matches_of(entry, q), None, g, n_groups, 9000)
            order = whole[2][:whole[0]].tolist()
            assert seen[i] == (order if done[i] else order[:len(seen[i])]), (entry, name, q)  # (a walk cut at 12 pages: the prefix)
        assert sum(done) >= 1 and pages >= 2
        x.close()
