"""Top values and distinct counts on the GPU through the C ABI (dint_ranked_or_top_values_queries,
dint_ranked_and_top_values_queries): every query's count of valued matches, count of different values and
top list equal to the model's (tests/top_values.py: np.unique and a lexsort), the count of valued matches equal to the percentile
entry's, and counts, scores, docids, matches and blocks_decoded equal to the filtered entry's on the same arguments, byte for
byte. The index is the hand-made one of tests/test_gpu_value_stats.py — 9 000 documents, a = 0 .. 2999, b = 5000 .. 8999, c = the
evens, d = every document (36 pages, the last one of 40 live slots), e = {10, 20, 30, 40}, and a sixth list that is empty. k = 10.
Everything is an integer: no tolerance anywhere. No call here may return the table-overflow status (every call goes through the
binding, which raises on any status but 0, or compares its status itself)."""
import ctypes as C

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import top_values as TV
from dint_amd import host
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import HAND_DOCS
from test_gpu_paging import CLUSTERED
from test_gpu_percentiles import Percentiles
from test_gpu_ranked_queries import _hand_made
from test_gpu_value_stats import EMPTY_LIST, QUERIES, _many_queries, edges_of

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")
M32 = 0xFFFFFFFF
K = 10
MEDIAN = [500000]


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


class TopValues(Percentiles):
    """Percentiles (an index, its freqs dictionary and wand data on the device, the filtered, value-stats and percentile entries
    and the model's matches) with the two top-values entries and their model."""

    def run_t(self, entry, qs, col, n_top, f, k=K):
        """-> (counts, scores, docids, matches, blocks_decoded, value_counts, distinct_counts, top_n, top_values, top_counts)"""
        fn = self.qi.ranked_or_top_values_queries if entry == "or" else self.qi.ranked_and_top_values_queries
        return fn(self.fd, self.wand, qs, col, n_top, filter=f, k=k)

    def want_t(self, entry, qs, values, n_top, mask):
        return TV.stacked([TV.top_values(self.matches_of(entry, q), mask, values, n_top) for q in qs], n_top)

    def check_t(self, entry, qs, values, col, n_top, k=K, mask=None, f=None, what=None):
        """the top-values call against the filtered entry on the same arguments — byte for byte, blocks_decoded too —, its count
        of valued matches against the percentile entry's, everything against the model; twice: the two runs are byte-identical"""
        what = (entry, n_top, k, what)
        got = self.run_t(entry, qs, col, n_top, f, k)
        same = self.run_f(entry, qs, f, k)
        _bit_equal(got[:4], same[:4], what)
        assert got[4] == same[4], what
        assert got[8].shape == got[9].shape == (len(qs), n_top), what
        _bit_equal((got[5],), (self.run_p(entry, qs, col, MEDIAN, f, k, stats=False)[3],), what)
        _bit_equal(got[5:], self.want_t(entry, qs, values, n_top, mask), what)
        again = self.run_t(entry, qs, col, n_top, f, k)
        _bit_equal(again[:4] + again[5:], got[:4] + got[5:], what)
        assert again[4] == got[4], what
        return got


@pytest.fixture(scope="module")
def hand(device):
    """the hand-made index with one list more, which no block names, made as tests/test_gpu_percentiles.py makes it"""
    import ranked

    kind = host.MULTI_PACKED
    r = TopValues(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    qi, wider = r.qi, C.c_void_p()
    assert device._lib.dint_query_index_create(qi.docs_dict._h, qi._index_dev.data_ptr(), qi._index_dev.numel(), qi.blocks.ctypes.data,
                                               len(qi.blocks), qi.n_lists + 1, C.byref(wider)) == 0
    qi.close()
    qi._h, qi.n_lists = wider, qi.n_lists + 1
    r.lists = ranked.BuilderLists(r.ix.docids, r.ix.freqs, np.append(r.ix.bounds, r.ix.bounds[-1]))
    assert r.lists.postings(EMPTY_LIST)[0].size == 0
    yield r
    r.close()


def hand_columns():
    return TV.named_columns(HAND_DOCS)


@pytest.fixture(scope="module")
def columns(device):
    cols = {name: (v, device.DocValues(0, v)) for name, v in hand_columns().items()}
    yield cols
    for _, c in cols.values():
        c.close()


# ---- the queries and the columns ----------------------------------------------------------------------------------------
def test_the_cases_are_what_they_are_said_to_be(hand):
    sizes = {e: [hand.matches_of(e, q)[1].size for q in QUERIES] for e in ENTRIES}
    for e in ENTRIES:
        assert [] in QUERIES and sizes[e][QUERIES.index([])] == 0 and sizes[e][QUERIES.index([EMPTY_LIST])] == 0
        assert sizes[e][QUERIES.index([3])] == HAND_DOCS and HAND_DOCS % 256 == 40  # 36 pages, the last one of 40 live slots
        assert sizes[e][QUERIES.index([4])] == 4 and any(s > 256 for s in sizes[e])
    cols = hand_columns()
    every = hand.matches_of("or", [3])
    # all distinct on the every-document query: 9 000 values in a table of 36 * 512 = 18 432 words, as full as a table gets
    assert TV.top_values(every, None, cols["v = d"], 3)[:2] == (HAND_DOCS, HAND_DOCS) and 2 * HAND_DOCS <= 36 * 512 < 2 * HAND_DOCS + 512
    ties = TV.top_values(every, None, cols["d % 1000"], 1024)
    assert ties[1:3] == (1000, 1000) and (ties[4][:1000] == 9).all()
    assert TV.top_values(every, None, cols["0 and ones"], 2)[3].tolist() == [0, M32]
    assert TV.N_TOPS == (0, 1, 3, 10, 256, 257, 1024)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(hand_columns()))
def test_columns_and_top_counts(hand, columns, entry, name):
    values, col = columns[name]
    for n_top in TV.N_TOPS:
        got = hand.check_t(entry, QUERIES, values, col, n_top, what=name)
        if name == "empty":
            assert not got[5].any() and not got[6].any() and not got[7].any() and not got[8].any() and not got[9].any()
    f = hand.filter(CLUSTERED)
    for n_top in (0, 10, 257):
        hand.check_t(entry, QUERIES, values, col, n_top, mask=CLUSTERED, f=f, what=(name, "clustered"))
    f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, columns, entry):
    values, col = columns["d % 1000"]
    for k in (1, 1024):
        for n_top in (0, 10, 1024):
            got = hand.check_t(entry, QUERIES, values, col, n_top, k=k)
    assert int(got[0].max()) == 1024 and int(got[5].max()) > 1024  # (the top values are over every match, not the top k)


# ---- filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_filters(hand, columns, entry):
    values, col = columns["d // 100"]
    # a value-range filter from the same column: every top value lies in [lo, hi]
    lo, hi = 29, 53
    f = hand.qi.doc_filter_from_values(col, lo, hi)
    got = hand.check_t(entry, QUERIES, values, col, 10, mask=DV.values_mask(values, lo, hi), f=f, what="value range")
    listed = np.arange(10)[None, :] < got[7][:, None]
    assert listed.any() and (got[8][listed] >= lo).all() and (got[8][listed] <= hi).all() and int(got[6].max()) == hi - lo + 1
    f.close()
    # a bitmap filter, and under it a column shorter than the index
    other, ocol = columns["half"]
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    hand.check_t(entry, QUERIES, values, col, 256, mask=mask, f=f, what="a bitmap")
    hand.check_t(entry, QUERIES, other, ocol, 256, mask=mask, f=f, what="a bitmap, a short column")
    f.close()
    # the empty filter: no valued match, nothing decoded
    nobody = np.zeros(HAND_DOCS, dtype=bool)
    f = hand.filter(nobody)
    got = hand.check_t(entry, QUERIES, values, col, 3, mask=nobody, f=f, what="empty")
    assert got[4] == 0 and not got[3].any() and not any(x.any() for x in got[5:])
    f.close()


# ---- batches, passes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_batch_and_one_query_per_call(hand, columns, entry):
    qs = _many_queries(300)
    assert [] in qs and len({tuple(q) for q in qs}) > 100
    for name, n_top in (("wide", 3), ("d % 7", 10)):
        values, col = columns[name]
        batch = hand.check_t(entry, qs, values, col, n_top, what=("batch", name))
        for i, q in enumerate(qs):
            one = hand.run_t(entry, [q], col, n_top, None)
            _bit_equal([x[0] for x in one[:4] + one[5:]], [x[i] for x in batch[:4] + batch[5:]], (entry, name, i))


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, hand, columns, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: the tables of later passes reuse the workspace, and their counters and
    selected keys lie at their own offset (the pass's first query)."""
    qs = _many_queries(60, seed=9) + QUERIES
    device.set_option("query_or_pass_pages", pass_pages)
    f = hand.filter(CLUSTERED)
    for name, n_top in (("wide", 257), ("d // 100", 10), ("v = d", 0)):
        values, col = columns[name]
        for entry in ENTRIES:
            got = hand.check_t(entry, qs, values, col, n_top, what=name)
            back = hand.run_t(entry, qs[::-1], col, n_top, None)
            _bit_equal([x[::-1] for x in back[5:]], got[5:], (entry, name, "reversed"))
            hand.check_t(entry, qs, values, col, n_top, mask=CLUSTERED, f=f, what=(name, "clustered"))
        assert int(got[6][len(qs) // 2:].sum()) > 0  # (queries of later passes have values)
    f.close()


# ---- errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, columns, entry):
    call = getattr(device._lib, f"dint_ranked_{entry}_top_values_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    values, col = columns["v = d"]

    def attempt(k, terms_, filt, col_, n_top=3, null=(), offs_=offs):
        counts, matches = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
        vc, dc, tn = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint32)
        scores, docids = np.full(1025, -1.0, dtype=np.float32), np.full(1025, 77, dtype=np.uint32)
        tv, tc = np.full(1025, 77, dtype=np.uint32), np.full(1025, 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        ptr = lambda name, a: None if name in null else a.ctypes.data  # noqa: E731
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  col_._h if col_ is not None else None, n_top, 1, ptr("counts", counts), matches.ctypes.data, scores.ctypes.data,
                  docids.ctypes.data, ptr("vc", vc), ptr("dc", dc), ptr("tn", tn), ptr("tv", tv), ptr("tc", tc), C.byref(blocks), None)
        untouched = (counts[0] == 77 and matches[0] == 77 and vc[0] == 77 and dc[0] == 77 and tn[0] == 77 and (scores == -1.0).all()
                     and (docids == 77).all() and (tv == 77).all() and (tc == 77).all() and blocks.value == 77)
        return st, untouched

    for filt in (None, f):
        assert attempt(0, terms, filt, col) == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, col) == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 6], dtype=np.uint32), filt, col) == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, col, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)  # decreasing offsets
        assert attempt(10, terms, filt, col, null=("counts",)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, None) == (DINT_ERR_ARG, True)  # no column
        assert attempt(10, terms, filt, col, n_top=1025) == (DINT_ERR_ARG, True)
        for name in ("vc", "dc", "tn", "tv", "tc"):
            assert attempt(10, terms, filt, col, null=(name,)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, n_top=1, null=("tv",)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, n_top=0, null=("vc",)) == (DINT_ERR_ARG, True)
    assert attempt(10, terms, f_other, col) == (DINT_ERR_ARG, True)  # a filter of another query index
    if device.device_count() > 1:  # a column on another device than the index (one device: this case alone is left out)
        elsewhere = device.DocValues(1, values)
        assert attempt(10, terms, None, elsewhere) == (DINT_ERR_ARG, True)
        elsewhere.close()
    st, untouched = attempt(10, terms, f, col)
    assert st == 0 and not untouched
    st, untouched = attempt(10, terms, f, col, n_top=0, null=("tv", "tc"))  # the counts only: no top arrays needed
    assert st == 0 and not untouched
    st, untouched = attempt(10, terms, None, col, n_top=1024)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_t(entry, [[6]], col, 3, f)
    with pytest.raises(device.DintError):
        hand.run_t(entry, [[0]], col, 3, f_other)
    with pytest.raises(device.DintError):
        hand.run_t(entry, [[0]], col, 1025, None)
    f_other.close()
    other.close()
    f.close()


# ---- beside the percentile calls ----------------------------------------------------------------------------------------
def test_top_values_and_percentile_calls_in_turn(hand, columns):
    """the workspaces are separate and grow: a top-values call, a percentile call and a top-values call again on one index, longer
    and shorter batches and other n_top in between, leave every answer correct"""
    values, col = columns["wide"]
    spread = [i * 1000000 // 15 for i in range(16)]
    many = _many_queries(120, seed=3)
    for entry in ENTRIES:
        hand.check_t(entry, QUERIES, values, col, 10)
        hand.check_p(entry, QUERIES, values, col, spread)
        hand.check_t(entry, QUERIES[::-1], values, col, 1024)
        hand.check_t(entry, [[4], [], [0, 1]], values, col, 3)
        hand.check_v(entry, QUERIES, values, col, edges_of(values, 16))
        hand.check_t(entry, many, values, col, 257)
        hand.check_p(entry, [[3]], values, col, MEDIAN)
        hand.check_t(entry, [[3]], values, col, 0)
        hand.check_t(entry, QUERIES, values, col, 256)
