"""Value statistics and range histograms on the GPU through the C ABI (dint_ranked_or_value_stats_queries,
dint_ranked_and_value_stats_queries): every query's record, bucket row and hit values equal to the model's
(tests/value_stats.py), and counts, scores, docids, matches and blocks_decoded equal to the filtered entry's on the same
arguments, byte for byte. The index is the hand-made one of the range, facet and doc-values tests — 9 000 documents, a =
0 .. 2999, b = 5000 .. 8999, c = the evens, d = every document (36 pages, the last one of 40 live slots), e = {10, 20, 30, 40} —
with a sixth list that is empty. k = 10. Everything is an integer: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import facets as FA
import ranked
import value_stats as VS
from dint_amd import host
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import HAND_DOCS, Faceted
from test_gpu_paging import CLUSTERED
from test_gpu_ranked_queries import _hand_made
from test_gpu_ranked_range import HAND_QUERIES

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")
M32 = 0xFFFFFFFF
K = 10
EDGE_COUNTS = (0, 1, 2, 255, 256, 257, 1023)  # around the flush loop's stride of 256, and every step count of the search up to ten
EMPTY_LIST = 5
QUERIES = HAND_QUERIES + [[EMPTY_LIST], [EMPTY_LIST, 0], [3, EMPTY_LIST], [4, 3, 3]]


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


def _same(got, want, what=None):
    """_bit_equal, None against None"""
    for g, w in zip(got, want):
        if g is None or w is None:
            assert g is None and w is None, what
        else:
            _bit_equal((g,), (w,), what)


class Stats(Faceted):
    """Faceted (an index, its freqs dictionary and wand data on the device, the filtered and faceted entries and the model's
    matches) with the two value-stats entries and their model."""

    def run_v(self, entry, qs, col, edges, f, k=K, stats=True):
        """-> (counts, scores, docids, matches, blocks_decoded, stats, buckets, hit_values); without the stats no matches and blocks"""
        fn = self.qi.ranked_or_value_stats_queries if entry == "or" else self.qi.ranked_and_value_stats_queries
        return fn(self.fd, self.wand, qs, col, edges=edges, filter=f, k=k, with_stats=stats)

    def want_v(self, entry, qs, values, edges, mask, k=K):
        return VS.stacked([VS.value_stats(self.matches_of(entry, q), mask, values, edges, k) for q in qs], k, len(edges))

    def check_v(self, entry, qs, values, col, edges, k=K, mask=None, f=None, what=None):
        """the value-stats call against the filtered entry on the same arguments — byte for byte, blocks_decoded too — and its
        records, rows and hit values against the model; twice: the two runs are byte-identical"""
        what = (entry, len(edges), k, what)
        got = self.run_v(entry, qs, col, edges, f, k)
        same = self.run_f(entry, qs, f, k)
        _bit_equal(got[:4], same[:4], what)
        assert got[4] == same[4], what
        _same(got[5:], self.want_v(entry, qs, values, edges, mask, k), what)
        if len(edges):
            assert got[6].shape == (len(qs), len(edges) + 1) and np.array_equal(got[6].sum(axis=1, dtype=np.uint64), got[5]["n"]), what
        past = [int((VS.matches_in(self.matches_of(entry, q), mask)[1] >= len(values)).sum()) for q in qs]
        assert (got[3] - got[5]["n"]).tolist() == past, what  # matches - n: the matches past the column
        again = self.run_v(entry, qs, col, edges, f, k)
        _same(again[:4] + again[5:], got[:4] + got[5:], what)
        assert again[4] == got[4], what
        return got


@pytest.fixture(scope="module")
def hand(device):
    """the hand-made index with one list more, which no block names: the index builder cannot write an empty list, so the
    handle is made again through the bare entry over the same index and block table (as tests/test_gpu_ranked_or_bool.py does)"""
    kind = host.MULTI_PACKED
    r = Stats(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
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
    return VS.named_columns(HAND_DOCS)


@pytest.fixture(scope="module")
def columns(device):
    cols = {name: (v, device.DocValues(0, v)) for name, v in hand_columns().items()}
    yield cols
    for _, c in cols.values():
        c.close()


def edges_of(values, n: int):
    """n strictly ascending edges for a column: 0 and 0xFFFFFFFF among them (n >= 2), then values the column holds, taken at
    even steps through it, then evenly spaced ones"""
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    have = [0, M32][:n] if n >= 2 else [int(values[len(values) // 2]) if len(values) else 7]
    pool = np.unique(np.asarray(values)[::max(1, len(values) // (2 * n))]).tolist() + VS.evenly(VS.MAX_EDGES, 1, M32 - 1).tolist()
    for x in pool:
        if len(have) == n:
            break
        if x not in have:
            have.append(int(x))
    assert len(have) == n
    return np.array(sorted(have), dtype=np.uint32)


# ---- the queries and the columns ----------------------------------------------------------------------------------------
def test_the_cases_are_what_they_are_said_to_be(hand):
    cols = hand_columns()
    sizes = {e: [hand.matches_of(e, q)[1].size for q in QUERIES] for e in ENTRIES}
    for e in ENTRIES:
        assert [] in QUERIES and sizes[e][QUERIES.index([])] == 0 and sizes[e][QUERIES.index([EMPTY_LIST])] == 0
        assert sizes[e][QUERIES.index([3])] == HAND_DOCS and HAND_DOCS % 256 == 40  # 36 pages, the last one of 40 live slots
        assert sizes[e][QUERIES.index([4])] == 4 and any(s > 256 for s in sizes[e])
    assert sizes["or"][QUERIES.index([EMPTY_LIST, 0])] == 3000 and sizes["and"][QUERIES.index([EMPTY_LIST, 0])] == 0
    assert [0, 0] in QUERIES and [2, 0, 2] in QUERIES  # a repeated term
    assert cols["half"].size == HAND_DOCS // 2 and cols["top + 3"].size == HAND_DOCS + 3 and cols["empty"].size == 0
    assert not cols["zeros"].any() and (cols["ones"] == M32).all() and (np.diff(cols["v = d"].astype(np.int64)) == 1).all()
    # the wide column: a handful of matches push the sum past 2^32
    four = VS.value_stats(hand.matches_of("or", [4]), None, cols["wide"], [], K)[0]
    assert four[0] == 4 and four[1] >= 1 << 32
    for n in EDGE_COUNTS:
        for name, v in cols.items():
            e = edges_of(v, n)
            assert e.size == n and (np.diff(e.astype(np.int64)) > 0).all() and (n < 2 or (e[0] == 0 and e[-1] == M32))
            assert n < 255 or name in ("zeros", "ones", "empty") or np.isin(e, v).sum() > 1  # edges equal to present values
    assert [max(0, n.bit_length()) for n in EDGE_COUNTS] == [0, 1, 2, 8, 9, 9, 10]  # the search's steps


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(hand_columns()))
def test_columns_and_edge_counts(hand, columns, entry, name):
    values, col = columns[name]
    populated = 0
    for n in EDGE_COUNTS:
        got = hand.check_v(entry, QUERIES, values, col, edges_of(values, n), what=name)
        populated = max(populated, int((got[6] != 0).sum(axis=1).max()) if got[6] is not None else 0)
    f = hand.filter(CLUSTERED)
    for n in (2, 257):
        hand.check_v(entry, QUERIES, values, col, edges_of(values, n), mask=CLUSTERED, f=f, what=(name, "clustered"))
    f.close()
    if name in ("v = d", "reverse", "wide"):
        assert populated > 256, populated  # (a query that fills more buckets than the workgroup has threads)
    short = hand.run_v(entry, QUERIES, col, edges_of(values, 2), None, stats=False)  # (without the stats: the same, three fewer)
    assert len(short) == 6 and short[3].dtype == VS.STATS_DTYPE


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, columns, entry):
    values, col = columns["wide"]
    for k in (1, 1024):
        got = hand.check_v(entry, QUERIES, values, col, edges_of(values, 16), k=k)
    assert int(got[0].max()) == 1024 and int(got[5]["n"].max()) > 1024  # (the records are over every match, not the top k)


# ---- filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_filters(hand, columns, entry):
    values, col = columns["v = d"]
    edges = edges_of(values, 255)
    # a value-range filter from the same column: every valued match lies in [lo, hi], and so do min and max
    lo, hi = 2900, 5300
    f = hand.qi.doc_filter_from_values(col, lo, hi)
    got = hand.check_v(entry, QUERIES, values, col, edges, mask=DV.values_mask(values, lo, hi), f=f, what="value range")
    some = got[5]["n"] > 0
    assert some.any() and (got[5]["min"][some] >= lo).all() and (got[5]["max"][some] <= hi).all()
    f.close()
    # ... and from another column, shorter than the index
    other, ocol = columns["half"]
    f = hand.qi.doc_filter_from_values(ocol, 300, 9000)
    hand.check_v(entry, QUERIES, values, col, edges, mask=DV.values_mask(other, 300, 9000), f=f, what="another column's range")
    f.close()
    # the empty filter: empty records, rows of zeros, nothing decoded
    nobody = np.zeros(HAND_DOCS, dtype=bool)
    f = hand.filter(nobody)
    got = hand.check_v(entry, QUERIES, values, col, edges, mask=nobody, f=f, what="empty")
    assert got[4] == 0 and not got[3].any() and not got[6].any() and not got[7].any()
    assert got[5].tobytes() == np.array([VS.EMPTY] * len(QUERIES), dtype=VS.STATS_DTYPE).tobytes()
    f.close()


# ---- batches, passes ----------------------------------------------------------------------------------------------------
def _many_queries(n, seed=4):
    r = np.random.default_rng(seed)
    return [r.integers(0, EMPTY_LIST + 1, int(r.integers(0, 5))).tolist() for _ in range(n)]


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_batch_and_one_query_per_call(hand, columns, entry):
    qs = _many_queries(300)
    assert [] in qs and len({tuple(q) for q in qs}) > 100
    for name, n in (("wide", 16), ("v = d", 1023)):
        values, col = columns[name]
        edges = edges_of(values, n)
        batch = hand.check_v(entry, qs, values, col, edges, what=("batch", name))
        for i, q in enumerate(qs):
            one = hand.run_v(entry, [q], col, edges, None)
            _same([x[0] for x in one[:4] + one[5:]], [x[i] for x in batch[:4] + batch[5:]], (entry, name, i))


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, hand, columns, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: the records, rows and hit values of the queries of later passes lie at
    their own offset (the pass's first query), and every pass adds to workspaces that were cleared once."""
    qs = _many_queries(60, seed=9) + QUERIES
    device.set_option("query_or_pass_pages", pass_pages)
    f = hand.filter(CLUSTERED)
    for name, n in (("wide", 2), ("v = d", 257)):
        values, col = columns[name]
        edges = edges_of(values, n)
        for entry in ENTRIES:
            got = hand.check_v(entry, qs, values, col, edges, what=name)
            back = hand.run_v(entry, qs[::-1], col, edges, None)
            _same([x[::-1] for x in back[5:]], got[5:], (entry, name, "reversed"))
            hand.check_v(entry, qs, values, col, edges, mask=CLUSTERED, f=f, what=(name, "clustered"))
        assert int(got[5]["n"][len(qs) // 2:].sum()) > 0  # (queries of later passes match something)
    f.close()


# ---- hit values ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_hit_values_without_docids_and_past_a_short_column(device, hand, columns, entry):
    values, col = columns["half"]  # 4500 documents: every hit of b = 5000 .. 8999 lies past it
    edges = edges_of(values, 2)
    got = hand.check_v(entry, QUERIES, values, col, edges, what="half")
    b = QUERIES.index([1])
    assert got[3][b] == 4000 and got[5][b].tolist() == VS.EMPTY and not got[7][b].any() and not got[6][b].any()
    d = QUERIES.index([3])  # every document: the first ten have their values, and half of the matches none
    assert got[7][d].tolist() == values[:K].tolist() and got[5]["n"][d] == 4500 and got[3][d] == HAND_DOCS
    # docids null while hit_values is not; then hit_values null; then neither matches nor blocks_decoded
    terms, offs = device._pack_queries(QUERIES)
    n = len(QUERIES)
    fn = getattr(device._lib, f"dint_ranked_{entry}_value_stats_queries")
    for with_docids, with_hits in ((False, True), (True, False), (False, False)):
        counts, matches = np.full(n, 77, dtype=np.uint64), np.full(n, 77, dtype=np.uint64)
        scores, docids, hv = np.full((n, K), -1.0, dtype=np.float32), np.full((n, K), 77, dtype=np.uint32), np.full((n, K), 77, dtype=np.uint32)
        stats, rows = np.full(n, 77, dtype=VS.STATS_DTYPE), np.full((n, 3), 77, dtype=np.uint32)
        st = fn(hand.qi._h, hand.fd._h, hand.wand._h, K, terms.ctypes.data, offs.ctypes.data, None, col._h, edges.ctypes.data, 2, n,
                counts.ctypes.data, matches.ctypes.data if with_docids else None, scores.ctypes.data, docids.ctypes.data if with_docids else None,
                stats.ctypes.data, rows.ctypes.data, hv.ctypes.data if with_hits else None, None, None)
        assert st == 0
        _bit_equal((counts, scores, stats, rows), (got[0], got[1], got[5], got[6]), (entry, with_docids, with_hits))
        assert (docids.tobytes() == got[2].tobytes() and matches.tobytes() == got[3].tobytes()) if with_docids else ((docids == 77).all() and (matches == 77).all())
        assert hv.tobytes() == got[7].tobytes() if with_hits else (hv == 77).all()
    # n_edges == 0: edges and bucket_counts are ignored and may be null
    counts, scores, stats = np.zeros(n, dtype=np.uint64), np.zeros((n, K), dtype=np.float32), np.full(n, 77, dtype=VS.STATS_DTYPE)
    assert fn(hand.qi._h, hand.fd._h, hand.wand._h, K, terms.ctypes.data, offs.ctypes.data, None, col._h, None, 0, n, counts.ctypes.data, None,
              scores.ctypes.data, None, stats.ctypes.data, None, None, None, None) == 0
    _bit_equal((counts, scores, stats), (got[0], got[1], got[5]), entry)


# ---- errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, columns, entry):
    call = getattr(device._lib, f"dint_ranked_{entry}_value_stats_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    values, col = columns["v = d"]
    e3 = np.array([10, 50, 200], dtype=np.uint32)

    def attempt(k, terms_, filt, col_, edges=e3, n_edges=3, null=(), offs_=offs):
        counts, matches = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
        scores, docids, hv = np.full(1025, -1.0, dtype=np.float32), np.full(1025, 77, dtype=np.uint32), np.full(1025, 77, dtype=np.uint32)
        stats, rows = np.full(1, 77, dtype=VS.STATS_DTYPE), np.full(1024, 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  col_._h if col_ is not None else None, edges.ctypes.data if edges is not None else None, n_edges, 1,
                  None if "counts" in null else counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                  None if "stats" in null else stats.ctypes.data, None if "rows" in null else rows.ctypes.data, hv.ctypes.data, C.byref(blocks), None)
        untouched = (counts[0] == 77 and matches[0] == 77 and (scores == -1.0).all() and (docids == 77).all() and (hv == 77).all()
                     and (rows == 77).all() and stats.tobytes() == np.full(1, 77, dtype=VS.STATS_DTYPE).tobytes() and blocks.value == 77)
        return st, untouched

    for filt in (None, f):
        assert attempt(0, terms, filt, col) == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, col) == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 6], dtype=np.uint32), filt, col) == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, col, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)  # decreasing offsets
        assert attempt(10, terms, filt, col, null=("counts",)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, None) == (DINT_ERR_ARG, True)  # no column
        assert attempt(10, terms, filt, col, null=("stats",)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, null=("rows",)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, edges=None) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, edges=np.arange(1024, dtype=np.uint32), n_edges=1024) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, edges=np.array([5, 5, 9], dtype=np.uint32)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, col, edges=np.array([7, 3, 9], dtype=np.uint32)) == (DINT_ERR_ARG, True)
    assert attempt(10, terms, f_other, col) == (DINT_ERR_ARG, True)  # a filter of another query index
    if device.device_count() > 1:  # a column on another device than the index (one device: this case alone is left out)
        elsewhere = device.DocValues(1, values)
        assert attempt(10, terms, None, elsewhere) == (DINT_ERR_ARG, True)
        elsewhere.close()
    st, untouched = attempt(10, terms, f, col)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_v(entry, [[6]], col, e3, f)
    with pytest.raises(device.DintError):
        hand.run_v(entry, [[0]], col, e3, f_other)
    with pytest.raises(ValueError):
        hand.run_v(entry, [[0]], col, [7, 3], f)
    f_other.close()
    other.close()
    f.close()


# ---- beside the faceted calls -------------------------------------------------------------------------------------------
def test_faceted_and_value_stats_calls_in_turn(hand, columns):
    """the two workspaces are separate: a faceted call, a value-stats call and a faceted call again on one index, longer and
    shorter batches in between, leave every answer correct"""
    values, col = columns["wide"]
    g = FA.named_map("striped", HAND_DOCS, 300)
    x = hand.facets(g, 300)
    for entry in ENTRIES:
        hand.check_x(entry, QUERIES, g, 300, facets=x)
        hand.check_v(entry, QUERIES, values, col, edges_of(values, 257))
        hand.check_x(entry, QUERIES[::-1], g, 300, facets=x)
        hand.check_v(entry, [[4], [], [0, 1]], values, col, edges_of(values, 1023))
        hand.check_v(entry, QUERIES[::-1], values, col, edges_of(values, 1))
        hand.check_x(entry, [[4]], g, 300, facets=x)
    x.close()
