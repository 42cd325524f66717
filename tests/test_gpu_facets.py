"""Faceted ranked queries on the GPU through the C ABI (dint_doc_facets_create, dint_ranked_or_faceted_queries,
dint_ranked_and_faceted_queries): the handle's group sizes exact; counts, matches, BM25 scores, docIDs and
blocks_decoded bit-equal to the filtered entries' on the same arguments; the facet rows equal to the model's (tests/facets.py:
numpy.bincount over the groups of the model's matches), their sum plus the matches in no group equal to matches."""
import ctypes as C
import threading

import numpy as np
import pytest

import doc_filter as DF
import facets as FA
import ranked
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_doc_filter import Filtered, _bit_equal
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import _hand_made
from test_gpu_ranked_range import HAND_QUERIES
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]
ENTRIES = ("or", "and")
HAND_DOCS = 9000
BOTH_FORMS = (256, 257)  # n_groups on both sides of the threshold between the LDS form and the global form
MAP_MAX_DOCS = 1 << 22   # (the sparse corpus spans 1.3e9 docIDs: the batch maps end here, every document past them is in no group)


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


class Faceted(Filtered):
    """Filtered (an index, its freqs dictionary and wand data on the device, the filtered entries and the model's matches)
    with the two faceted entries and the model's rows."""

    def __init__(self, device, *a, **kw):
        super().__init__(device, *a, **kw)
        self.device = device

    def facets(self, group_of, n_groups):
        return self.device.DocFacets(0, group_of, n_groups)

    def run_x(self, entry, qs, facets, f, k, stats=True):
        fn = self.qi.ranked_or_faceted_queries if entry == "or" else self.qi.ranked_and_faceted_queries
        return fn(self.fd, self.wand, qs, facets, filter=f, k=k, with_stats=stats)

    def want_rows(self, entry, qs, mask, group_of, n_groups):
        """-> (rows u32[n, n_groups], per query the matches in no group)"""
        out = [FA.row_of(group_of, n_groups, FA.matches_in(self.matches_of(entry, q), mask)) for q in qs]
        rows = np.stack([o[0] for o in out]) if out else np.zeros((0, n_groups), np.uint32)
        return rows, np.array([o[1] for o in out], dtype=np.int64)

    def check_x(self, entry, qs, group_of, n_groups, k=10, mask=None, f=None, facets=None, what=None):
        """the faceted call (through the handles given, or ones made and closed here) against the filtered entry on the same
        arguments — bit for bit, blocks_decoded too — and its rows against the model"""
        what = (entry, n_groups, k, what)
        own_f, own_x = f is None and mask is not None, facets is None
        if own_f:
            f = self.filter(mask)
        if own_x:
            facets = self.facets(group_of, n_groups)
        got = self.run_x(entry, qs, facets, f, k)
        same = self.run_f(entry, qs, f, k)
        _bit_equal(got[:4], same[:4], what)
        assert got[4] == same[4], what
        rows, none = self.want_rows(entry, qs, mask, group_of, n_groups)
        assert got[5].dtype == np.uint32 and got[5].shape == rows.shape, what
        assert np.array_equal(got[5], rows), what
        assert np.array_equal(got[5].sum(axis=1, dtype=np.int64) + none, got[3].astype(np.int64)), what
        short = self.run_x(entry, qs, facets, f, k, stats=False)  # (without the stats: the same, and the rows last)
        _bit_equal(short[:3], got[:3], what)
        assert np.array_equal(short[3], rows), what
        if own_f:
            f.close()
        if own_x:
            facets.close()
        return got


@pytest.fixture(scope="module")
def hand(device):
    """test_gpu_ranked_range.py's hand-made index: a = 0 .. 2999 (blocks [256 j, 256 j + 255], the last one 2816 .. 2999),
    b = 5000 .. 8999 (the last block is 8840 .. 8999), c = the evens, d = every doc (page j holds 256 j .. 256 j + 255: a
    document's lane is d & 63), e = {10, 20, 30, 40}"""
    kind = host.MULTI_PACKED
    r = Faceted(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    yield r
    r.close()


# ---- the handle ---------------------------------------------------------------------------------------------------------
def _check_handle(device, group_of, n_groups, what=None):
    x = device.DocFacets(0, group_of, n_groups)
    sizes, n_grouped = FA.sizes_of(group_of, n_groups)
    assert (x.num_docs, x.n_groups, x.n_grouped) == (len(group_of), n_groups, n_grouped), what
    assert x.group_sizes.dtype == np.uint32 and np.array_equal(x.group_sizes, sizes), what
    x.close()


# (256 documents are one workgroup of the group-size launch; the last size: several workgroups and a ragged last one)
@pytest.mark.parametrize("num_docs", [1, 63, 64, 65, 255, 256, 257, 5 * 256 + 77])
def test_group_sizes_are_exact(device, num_docs):
    for n_groups in (1, 2, 255, 256, 257, 65536):
        for name in FA.MAPS:
            _check_handle(device, FA.named_map(name, num_docs, n_groups, seed=num_docs), n_groups, (num_docs, n_groups, name))


def test_group_sizes_of_a_larger_map(device):
    n = 300 * 256 + 5
    for n_groups in (3, 256, 257, 65536):
        for name in FA.MAPS:
            _check_handle(device, FA.named_map(name, n, n_groups), n_groups, (n_groups, name))
    x = device.DocFacets(0, [], 4)  # no document: every group empty
    assert (x.num_docs, x.n_groups, x.n_grouped) == (0, 4, 0) and not x.group_sizes.any()
    x.close()
    x = device.DocFacets(0, [2, None, -7, 0, 2])  # the default n_groups: the largest group + 1
    assert (x.num_docs, x.n_groups, x.n_grouped) == (5, 3, 3) and x.group_sizes.tolist() == [1, 0, 2]
    x.close()


@pytest.mark.parametrize("n_groups", [1, 7, 256, 257, 65536])
def test_an_invalid_entry_gives_no_handle(device, n_groups):
    lib = device._lib
    for num_docs in (1, 300, 4 * 256 + 9):
        for at in sorted({0, num_docs // 2, num_docs - 1}):  # the first, a middle and the last position
            for bad in (n_groups, n_groups + 1, 0xFFFFFFFE):
                m = np.ascontiguousarray(FA.named_map("striped", num_docs, n_groups), dtype=np.uint32)
                m[at] = bad
                h = C.c_void_p(77)
                assert lib.dint_doc_facets_create(0, m.ctypes.data, num_docs, n_groups, C.byref(h)) == DINT_ERR_ARG, (num_docs, at, bad)
                assert h.value is None
                with pytest.raises(device.DintError):
                    device.DocFacets(0, m, n_groups)
            m = np.ascontiguousarray(FA.named_map("striped", num_docs, n_groups), dtype=np.uint32)
            m[at] = 0xFFFFFFFF  # (NONE there is no error)
            _check_handle(device, np.where(m == 0xFFFFFFFF, FA.NONE, m.astype(np.int64)), n_groups)


def test_group_counts_that_are_refused(device):
    m = np.zeros(10, dtype=np.uint32)
    for n_groups in (0, 65537, 1 << 20):
        h = C.c_void_p(77)
        assert device._lib.dint_doc_facets_create(0, m.ctypes.data, 10, n_groups, C.byref(h)) == DINT_ERR_ARG and h.value is None
        with pytest.raises(device.DintError):
            device.DocFacets(0, m, n_groups)
    _check_handle(device, np.zeros(10, dtype=np.int64), 65536)


# ---- kernel edges on the hand-made index --------------------------------------------------------------------------------
def _two(n, cut, hi):
    """documents below `cut` in group 0, the others in group hi"""
    g = np.zeros(n, dtype=np.int64)
    g[cut:] = hi
    return g


def hand_maps(n_groups):
    """{name: group_of}. Under query [3] (d, every document) document x sits in page x // 256, lane x & 63."""
    last = n_groups - 1
    none_between = np.full(HAND_DOCS, 3, dtype=np.int64)
    none_between[[100, 101, 127, 128, 2999]] = FA.NONE
    maps = {
        "a run ends at lane 62": _two(HAND_DOCS, 63, last),
        "a run ends at lane 63, the next begins a wave": _two(HAND_DOCS, 64, last),
        "a run ends at lane 62 of the page's last wave": _two(HAND_DOCS, 255, last),
        "a run ends at the page's last slot": _two(HAND_DOCS, 256, last),
        "a run of one at the page's last slot": np.where(np.arange(HAND_DOCS) % 256 == 255, 5, 0),
        "a run of one in lane 0": np.where(np.arange(HAND_DOCS) % 64 == 0, 5, 0),
        "every page of one group, group 0 in lane 0": np.zeros(HAND_DOCS, dtype=np.int64),
        "every page of the last group": np.full(HAND_DOCS, last, dtype=np.int64),
        "group 0 in lane 0 only": np.where(np.arange(HAND_DOCS) % 64 == 0, 0, last),
        "a NONE document between two of one group": none_between,
        "none": FA.named_map("none", HAND_DOCS, n_groups),
        "every other document NONE": FA.named_map("every other document NONE", HAND_DOCS, n_groups),
        "a group a document": np.arange(HAND_DOCS, dtype=np.int64) % n_groups,
        "runs of three": (np.arange(HAND_DOCS, dtype=np.int64) // 3) % n_groups,
        "runs of 64 from lane 1 on": ((np.arange(HAND_DOCS, dtype=np.int64) + 63) // 64) % n_groups,
        "clustered": FA.named_map("clustered", HAND_DOCS, n_groups),
        "random": FA.named_map("random", HAND_DOCS, n_groups),
        "a's short last block in a group of its own": np.where((np.arange(HAND_DOCS) >= 2816) & (np.arange(HAND_DOCS) < 3000), last, 1),
        "b's and d's short last block in a group of its own": np.where(np.arange(HAND_DOCS) >= 8840, last, 1),
        "the list of one block": np.where(np.isin(np.arange(HAND_DOCS), [10, 20, 30, 40]), np.arange(HAND_DOCS) // 10, FA.NONE),
        "the map ends inside a page": _two(5100, 63, last),      # (the matches at and past 5100 are in no group)
        "the map ends before the first match of b": _two(300, 64, last),
        "a map of one document": np.zeros(1, dtype=np.int64),
    }
    return maps


HAND_MAP_NAMES = list(hand_maps(300))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_groups", BOTH_FORMS)
@pytest.mark.parametrize("name", HAND_MAP_NAMES)
def test_kernel_edges(hand, entry, n_groups, name):
    """HAND_QUERIES under every hand-made map. Among them [3] (full pages of consecutive documents: the lanes are the
    documents'), [0] and [1] (short last blocks), [4] (a list of one block) and — a dead slot between two live ones of one
    group — [0, 2] (OR: c holds a's even documents, so in a's pages every other slot is a non-representative; AND: of a's
    candidates every other one survives) and [1, 2, 3]."""
    g = hand_maps(n_groups)[name]
    x = hand.facets(g, n_groups)
    got = hand.check_x(entry, HAND_QUERIES, g, n_groups, k=10, facets=x, what=name)
    for i in (2, 5, 6, 9, 10, 13):  # one query per call: the same rows
        one = hand.check_x(entry, [HAND_QUERIES[i]], g, n_groups, k=1000, facets=x, what=(name, i))
        assert np.array_equal(one[5][0], got[5][i]) and one[3][0] == got[3][i]
    x.close()


def test_the_edge_cases_are_what_they_are_said_to_be(hand):
    n_groups = 257
    maps = hand_maps(n_groups)
    last = n_groups - 1
    every = {q: hand.matches_of("or", [q])[1] for q in (0, 1, 3, 4)}
    assert every[3].tolist() == list(range(HAND_DOCS)) and every[4].tolist() == [10, 20, 30, 40]
    g = maps["a run ends at lane 62"]
    assert g[62] == 0 and g[63] == last
    g = maps["a run ends at the page's last slot"]
    assert g[255] == 0 and g[256] == last
    g = maps["a NONE document between two of one group"]
    assert g[99] == g[102] == 3 and g[100] == FA.NONE and g[127] == g[128] == FA.NONE  # (inside a wave, and across two)
    # the dead slot between two live ones: the union's representatives in a's pages are the odd documents, the
    # intersection's survivors the even ones
    rows, none = hand.want_rows("and", [[0, 2]], None, maps["clustered"], n_groups)
    assert int(rows.sum()) == 1500 and none[0] == 0
    # the short maps: the row falls short of the matches by exactly the matches past the map
    for name, n_map in (("the map ends inside a page", 5100), ("the map ends before the first match of b", 300), ("a map of one document", 1)):
        assert len(maps[name]) == n_map
        for entry in ENTRIES:
            got = hand.check_x(entry, HAND_QUERIES, maps[name], n_groups, what=name)
            past = np.array([int((FA.matches_in(hand.matches_of(entry, q), None) >= n_map).sum()) for q in HAND_QUERIES])
            assert np.array_equal(got[3].astype(np.int64) - got[5].sum(axis=1, dtype=np.int64), past) and past.sum() > 0
    got = hand.check_x("or", [[3], [1], []], maps["the map ends inside a page"], n_groups)
    assert got[3].tolist() == [9000, 4000, 0] and got[5].sum(axis=1).tolist() == [5100, 100, 0]
    assert got[5][0, 0] == 63 and got[5][0, last] == 5100 - 63 and not got[5][2].any()


@pytest.mark.parametrize("entry", ENTRIES)
def test_edges_under_a_filter(hand, entry):
    """the filter path: pages are the live blocks, and what they hold outside the filter is dead before it is counted"""
    for members in ([63, 64, 65], list(range(200, 600)) + [2999, 8999], list(range(0, HAND_DOCS, 3))):
        mask = DF.as_mask(members, HAND_DOCS)
        f = hand.filter(mask)
        for n_groups in BOTH_FORMS:
            for name in ("a run ends at lane 63, the next begins a wave", "a group a document", "clustered", "every other document NONE",
                         "the map ends inside a page"):
                hand.check_x(entry, HAND_QUERIES, hand_maps(n_groups)[name], n_groups, mask=mask, f=f, what=(name, len(members)))
        f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, entry):
    g = FA.named_map("striped", HAND_DOCS, 8)
    x = hand.facets(g, 8)
    for k in (1, 1024):
        got = hand.check_x(entry, HAND_QUERIES, g, 8, k=k, facets=x)
    assert int(got[0].max()) == 1024 and int(got[3].max()) > 1024
    assert int(got[5].sum(axis=1).max()) > 1024  # (the rows count every match, not the top k)
    x.close()


def test_two_calls_in_a_row_leave_no_stale_rows(hand):
    """one handle, different batches: a longer batch first, then shorter ones, other group counts in between — a row that
    the second call did not clear would show"""
    g8, g300 = FA.named_map("striped", HAND_DOCS, 8), FA.named_map("random", HAND_DOCS, 300)
    x8, x300 = hand.facets(g8, 8), hand.facets(g300, 300)
    for entry in ENTRIES:
        hand.check_x(entry, HAND_QUERIES, g8, 8, facets=x8)
        hand.check_x(entry, [[4], [], [0, 1]], g8, 8, facets=x8)
        hand.check_x(entry, HAND_QUERIES[::-1], g300, 300, facets=x300)
        hand.check_x(entry, [[], []], g300, 300, facets=x300)
        got = hand.check_x(entry, [[4]], g8, 8, facets=x8)
        assert got[5].tolist() == [[1, 0, 1, 0, 1, 0, 1, 0]]  # 10, 20, 30, 40 mod 8: 2, 4, 6, 0
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
    r = Faceted(device, ix, kind, every=_EVERY.setdefault(corpus_name, {}))
    qs = reference_queries(len(ix.lens))[::4] + heavy_queries(ix.lens, 10) + [[]]
    n_map = min(r.num_docs, MAP_MAX_DOCS)
    mask = DF.batch_filter("runs", DF.batch_num_docs(r.num_docs), ix.docids, None)
    f = r.filter(mask)
    counted = {e: 0 for e in ENTRIES}
    for name in FA.MAPS:
        for n_groups in (8, 1000):
            g = FA.named_map(name, n_map, n_groups)
            x = r.facets(g, n_groups)
            for entry in ENTRIES:
                got = r.check_x(entry, qs, g, n_groups, facets=x, what=(corpus_name, name))
                counted[entry] += int(got[5].sum())
                assert not got[5][-1].any() and got[3][-1] == 0  # the empty query inside the batch
                r.check_x(entry, qs, g, n_groups, mask=mask, f=f, facets=x, what=(corpus_name, name, "runs"))
            x.close()
    f.close()
    assert counted["or"] > 5000 and counted["and"] > 500, counted
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: the rows of the queries of later passes are counted at their own
    offset (the pass's first query), and every pass adds to rows that were cleared once."""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Faceted(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2) + [[], [0]]
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    device.set_option("query_or_pass_pages", pass_pages)
    for n_groups, name in ((8, "clustered"), (1000, "striped")):
        g = FA.named_map(name, r.num_docs, n_groups)
        x = r.facets(g, n_groups)
        for entry in ENTRIES:
            got = r.check_x(entry, qs, g, n_groups, facets=x, what=name)
            back = r.run_x(entry, qs[::-1], x, None, 10)
            assert np.array_equal(back[5][::-1], got[5]) and np.array_equal(back[3][::-1], got[3])
            r.check_x(entry, qs, g, n_groups, mask=mask, f=f, facets=x, what=(name, "runs"))
        assert int(got[5][len(qs) // 2:].sum()) > 0  # (queries of later passes match something)
        x.close()
    f.close()
    r.close()


# ---- docIDs at the top of the u32 range ---------------------------------------------------------------------------------
def test_docids_near_2_to_the_32_under_a_small_map(device):
    """An index with docIDs up to 0xFFFFFFFE under maps that end far below: every high document is past the map, which is
    never read past its end (the bound is compared first), and counts as a match in no group."""
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
    for n_map, n_groups in ((100, 7), (6, 300), (1000, 256), (1, 1)):
        g = FA.named_map("striped", n_map, n_groups)
        x = device.DocFacets(0, g, n_groups)
        for entry in ENTRIES:
            fn = qi.ranked_or_faceted_queries if entry == "or" else qi.ranked_and_faceted_queries
            plain = qi.ranked_or_filtered_queries if entry == "or" else qi.ranked_and_filtered_queries
            got = fn(h.fd, wand, qs, x, k=10, with_stats=True)
            _bit_equal(got[:4], plain(h.fd, wand, qs, None, k=10, with_stats=True)[:4], (n_map, entry))
            every = [FA.every_match(bl, q, nl, num_docs, entry == "and")[1] for q in qs]
            want = [FA.row_of(g, n_groups, ids) for ids in every]
            assert np.array_equal(got[5], np.stack([w[0] for w in want])), (n_map, entry)
            assert got[3].tolist() == [ids.size for ids in every]
            assert (got[3].astype(np.int64) - got[5].sum(axis=1, dtype=np.int64)).tolist() == [int((ids >= n_map).sum()) for ids in every]
        x.close()
    qi.close()
    wand.close()


# ---- errors, and two threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, entry):
    lib = device._lib
    call = getattr(lib, f"dint_ranked_{entry}_faceted_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    g = FA.named_map("striped", HAND_DOCS, 8)
    x = hand.facets(g, 8)

    def attempt(k, terms_, filt, fac, counts_null=False, rows_null=False, offs_=offs, n=1):
        counts = np.full(1, 77, dtype=np.uint64)
        matches = np.full(1, 77, dtype=np.uint64)
        scores = np.full(1025, -1.0, dtype=np.float32)
        docids = np.full(1025, 77, dtype=np.uint32)
        rows = np.full(16, 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  fac._h if fac is not None else None, n, None if counts_null else counts.ctypes.data, matches.ctypes.data,
                  scores.ctypes.data, docids.ctypes.data, None if rows_null else rows.ctypes.data, C.byref(blocks), None)
        untouched = (counts[0] == 77 and matches[0] == 77 and (scores == -1.0).all() and (docids == 77).all() and (rows == 77).all()
                     and blocks.value == 77)
        return st, untouched

    for filt in (None, f):
        assert attempt(0, terms, filt, x) == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, x) == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 5], dtype=np.uint32), filt, x) == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, x, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)  # decreasing offsets
        assert attempt(10, terms, filt, x, counts_null=True) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, None) == (DINT_ERR_ARG, True)               # no facets
        assert attempt(10, terms, filt, x, rows_null=True) == (DINT_ERR_ARG, True)  # nowhere for the rows
    assert attempt(10, terms, f_other, x) == (DINT_ERR_ARG, True)  # a filter of another query index
    # n_queries * n_groups past 2^28: refused before the offsets are read
    big = hand.facets(np.zeros(1, dtype=np.int64), 65536)
    assert attempt(10, terms, None, big, n=(1 << 12) + 1) == (DINT_ERR_ARG, True)
    big.close()
    st, untouched = attempt(10, terms, f, x)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_x(entry, [[5]], x, f, 10)
    with pytest.raises(device.DintError):
        hand.run_x(entry, [[0]], x, f_other, 10)
    # nullable outputs: matches, docids and blocks_decoded
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    rows = np.full(8, 77, dtype=np.uint32)
    assert call(hand.qi._h, hand.fd._h, hand.wand._h, 10, terms.ctypes.data, offs.ctypes.data, f._h, x._h, 1, counts.ctypes.data,
                None, scores.ctypes.data, None, rows.ctypes.data, None, None) == 0
    want = hand.want_f(entry, [[0, 1]], mask, 10)
    assert counts[0] == want[0][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))
    assert np.array_equal(rows, hand.want_rows(entry, [[0, 1]], mask, g, 8)[0][0])
    x.close()
    f_other.close()
    other.close()
    f.close()


def test_two_threads_one_index_one_facets_handle(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Faceted(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    g = FA.named_map("clustered", r.num_docs, 300)
    x = r.facets(g, 300)
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    want = {e: (r.want_f(e, qs, mask if e == "and" else np.ones(r.num_docs, dtype=bool), 10), r.want_rows(e, qs, mask if e == "and" else None, g, 300)[0])
            for e in ENTRIES}
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine = ENTRIES[which]
            for _ in range(3):
                got = r.run_x(mine, qs, x, f if mine == "and" else None, 10)
                _bit_equal(got[:4], want[mine][0])
                assert np.array_equal(got[5], want[mine][1])
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
