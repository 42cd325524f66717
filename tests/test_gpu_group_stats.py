"""Per-group value statistics on the GPU through the C ABI (dint_ranked_or_group_stats_queries,
dint_ranked_and_group_stats_queries): every (query, group) record equal to the model's
(tests/group_stats.py); counts, scores, docids, matches and blocks_decoded equal to the filtered entry's on the same arguments and
facet_counts to the faceted entry's, byte for byte. The index is the hand-made one of the facet and value-stats tests — 9 000
documents, a = 0 .. 2999, b = 5000 .. 8999, c = the evens, d = every document (36 pages, the last one of 40 live slots; a
document's lane is d & 63), e = {10, 20, 30, 40} — with a sixth list that is empty. k = 10. Everything is an integer: no
tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import facets as FA
import group_stats as GS
import ranked
from dint_amd import host
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import HAND_DOCS
from test_gpu_paging import CLUSTERED
from test_gpu_ranked_queries import _hand_made
from test_gpu_value_stats import EMPTY_LIST, QUERIES, Stats, _many_queries, edges_of

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")
M32 = 0xFFFFFFFF
K = 10


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


class Grouped:
    """Stats (an index, its freqs dictionary and wand data on the device, the filtered, faceted and value-stats entries and the
    model's matches) with the two group-stats entries and their model."""

    def __init__(self, stats: Stats):
        self.s, self.qi = stats, stats.qi

    def run_g(self, entry, qs, facets, col, f, k=K, rows=True):
        """-> (counts, scores, docids, matches, blocks_decoded, group_stats, facet_counts or None)"""
        fn = self.qi.ranked_or_group_stats_queries if entry == "or" else self.qi.ranked_and_group_stats_queries
        return fn(self.s.fd, self.s.wand, qs, facets, col, filter=f, k=k, with_facet_counts=rows)

    def want_g(self, entry, qs, group_of, n_groups, values, mask):
        return GS.stacked([GS.group_stats(self.s.matches_of(entry, q), mask, group_of, n_groups, values) for q in qs], n_groups)

    def check_g(self, entry, qs, group_of, n_groups, facets, values, col, k=K, mask=None, f=None, what=None):
        """the group-stats call against the filtered entry on the same arguments — byte for byte, blocks_decoded too —, its rows
        against the faceted entry's, and its records against the model; twice: the two runs are byte-identical"""
        what = (entry, n_groups, k, what)
        got = self.run_g(entry, qs, facets, col, f, k)
        same = self.s.run_f(entry, qs, f, k)
        _bit_equal(got[:4], same[:4], what)
        assert got[4] == same[4], what
        rows = self.s.run_x(entry, qs, facets, f, k)[5]
        _bit_equal((got[6],), (rows,), what)
        assert got[5].shape == (len(qs), n_groups) and got[5].dtype == GS.STATS_DTYPE, what
        _bit_equal((got[5],), (self.want_g(entry, qs, group_of, n_groups, values, mask),), what)
        # n <= the group's matches everywhere, equal where the column covers the index
        assert (got[5]["n"] <= got[6]).all() and (len(values) < HAND_DOCS or np.array_equal(got[5]["n"], got[6])), what
        again = self.run_g(entry, qs, facets, col, f, k)
        _bit_equal(again[:4] + again[5:], got[:4] + got[5:], what)
        assert again[4] == got[4], what
        return got


@pytest.fixture(scope="module")
def hand(device):
    """the hand-made index with one list more, which no block names, as tests/test_gpu_value_stats.py makes it"""
    kind = host.MULTI_PACKED
    r = Stats(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    qi, wider = r.qi, C.c_void_p()
    assert device._lib.dint_query_index_create(qi.docs_dict._h, qi._index_dev.data_ptr(), qi._index_dev.numel(), qi.blocks.ctypes.data,
                                               len(qi.blocks), qi.n_lists + 1, C.byref(wider)) == 0
    qi.close()
    qi._h, qi.n_lists = wider, qi.n_lists + 1
    r.lists = ranked.BuilderLists(r.ix.docids, r.ix.freqs, np.append(r.ix.bounds, r.ix.bounds[-1]))
    assert r.lists.postings(EMPTY_LIST)[0].size == 0
    yield Grouped(r)
    r.close()


@pytest.fixture(scope="module")
def columns(device):
    cols = {name: (v, device.DocValues(0, v)) for name, v in GS.named_columns(HAND_DOCS).items() if name in GS.COLUMNS}
    yield cols
    for _, c in cols.values():
        c.close()


class Maps:
    """the facets handles of the named maps, made once per (name, n_groups) and closed with the module"""

    def __init__(self, device):
        self.device, self.made = device, {}

    def of(self, name, n_groups):
        if (name, n_groups) not in self.made:
            g = GS.named_maps(HAND_DOCS, n_groups)[name]
            self.made[name, n_groups] = (g, self.device.DocFacets(0, g, n_groups))
        return self.made[name, n_groups]

    def close(self):
        for _, x in self.made.values():
            x.close()


@pytest.fixture(scope="module")
def maps(device):
    m = Maps(device)
    yield m
    m.close()


# ---- the cases are what they are said to be -----------------------------------------------------------------------------
def test_the_cases_are_what_they_are_said_to_be(hand):
    cols = GS.named_columns(HAND_DOCS)
    d = QUERIES.index([3])
    for e in ENTRIES:
        assert hand.s.matches_of(e, [3])[1].size == HAND_DOCS and HAND_DOCS % 256 == 40  # 36 pages, the last one of 40 live slots
        assert hand.s.matches_of(e, [EMPTY_LIST])[1].size == 0
    assert [] in QUERIES and d >= 0
    m = GS.named_maps(HAND_DOCS, 300)
    assert (np.diff(m["striped"]) != 0).all()  # runs of 1
    w = -(-HAND_DOCS // 300)
    assert w == 30 and (m["clustered"][:64] == np.arange(64) // 30).all()  # runs that cross the rows at 16, 32 and 48
    assert (m["runs of 5"][:20] == np.arange(20) // 5).all() and (m["one group"] == 299).all() and (m["none"] == FA.NONE).all()
    assert (m["every other document NONE"][1::2] == FA.NONE).all() and (m["every other document NONE"][::2] != FA.NONE).all()
    assert len(m["short"]) < HAND_DOCS < len(m["long"])
    lone = m["group 0 in lane 0 only"]
    assert lone[0] == 0 and (lone[1:] == 299).all()  # group 0 held by the document in lane 0, and absent from every other page
    wide = GS.named_maps(HAND_DOCS, 2)["clustered"]
    assert (wide[:4500] == 0).all() and (wide[4500:] == 1).all()  # runs of 64 that end with the wave, a group fed from 18 pages
    assert not cols["zeros"].any() and (cols["ones"] == M32).all() and cols["half"].size == HAND_DOCS // 2
    assert cols["top + 3"].size == HAND_DOCS + 3 and cols["empty"].size == 0
    # "ones" with one group: the sum is 9 000 * 0xFFFFFFFF, and a run of 64 already needs 38 bits
    one = GS.group_stats(hand.s.matches_of("or", [3]), None, GS.named_maps(HAND_DOCS, 1)["one group"], 1, cols["ones"])
    assert one.tolist() == [(HAND_DOCS, HAND_DOCS * M32, M32, M32)] and 64 * M32 >= 1 << 37
    # "half" ends at document 4500, inside a run of its group under the clustered maps of 7 groups (1286 documents each) and of
    # 259 (35 each): grouped but unvalued lanes in the run, in the LDS form and in the direct one
    assert cols["half"].size == 4500
    for n_groups in (7, 259):
        c = GS.named_maps(HAND_DOCS, n_groups)["clustered"]
        assert c[4498] == c[4499] == c[4500] == c[4501] and 4500 % 64 not in (0, 63)


# ---- the kernel's edges -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n_groups", GS.GROUP_COUNTS)
def test_group_counts_maps_and_columns(hand, maps, columns, entry, n_groups):
    """every named map at every group count against the wide column, and every named column against the clustered map"""
    values, col = columns["wide"]
    for name in GS.named_maps(HAND_DOCS, n_groups):
        group_of, x = maps.of(name, n_groups)
        got = hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, what=name)
        if name == "none":
            assert got[5].tobytes() == GS.empty_records(len(QUERIES), n_groups).tobytes() and not got[6].any()
    group_of, x = maps.of("clustered", n_groups)
    for name in GS.COLUMNS:
        values, col = columns[name]
        got = hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, what=name)
        d = QUERIES.index([3])
        if name == "zeros":  # n > 0 with min = max = 0 differs from the empty record
            assert got[5][d, 0].tolist() == (int(got[6][d, 0]), 0, 0, 0) and got[6][d, 0] > 0
        if name == "empty":
            assert got[5].tobytes() == GS.empty_records(len(QUERIES), n_groups).tobytes() and got[6].any()


@pytest.mark.parametrize("entry", ENTRIES)
def test_sums_past_32_bits_and_unvalued_lanes_inside_a_run(hand, maps, columns, entry):
    d = QUERIES.index([3])
    values, col = columns["ones"]
    group_of, x = maps.of("one group", 1)
    got = hand.check_g(entry, QUERIES, group_of, 1, x, values, col, what="ones, one group")
    assert got[5][d, 0].tolist() == (HAND_DOCS, HAND_DOCS * M32, M32, M32)
    for n_groups in (2, 300):  # the LDS table and the direct atomics
        group_of, x = maps.of("one group", n_groups)
        got = hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, what="ones, the last group")
        assert got[5][d, n_groups - 1].tolist() == (HAND_DOCS, HAND_DOCS * M32, M32, M32)
    values, col = columns["half"]
    for n_groups in (7, 259):
        group_of, x = maps.of("clustered", n_groups)
        got = hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, what="half, clustered")
        g = int(group_of[len(values)])  # the group whose run the column ends in: its minimum is a real value, not a lent 0
        assert 0 < got[5][d, g]["n"] < got[6][d, g] and got[5][d, g]["min"] == values[np.flatnonzero(group_of == g)[0]] > 0
        last = int(group_of[HAND_DOCS - 1])  # a group wholly past the column: counted, and its record empty
        assert got[5][d, last].tolist() == GS.EMPTY and got[6][d, last] > 0
    for name in ("every other document NONE", "runs of 5"):
        group_of, x = maps.of(name, 256)
        hand.check_g(entry, QUERIES, group_of, 256, x, values, col, what=("half", name))


# ---- filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_filters(hand, maps, columns, entry):
    values, col = columns["top + 3"]
    for n_groups in (7, 300):
        group_of, x = maps.of("clustered", n_groups)
        f = hand.s.filter(CLUSTERED)
        hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, mask=CLUSTERED, f=f, what="clustered")
        f.close()
        # a value-range filter from the same column: every contributing match lies in [lo, hi], and so do min and max
        lo, hi = 2900, 5300
        f = hand.qi.doc_filter_from_values(col, lo, hi)
        got = hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, mask=DV.values_mask(values, lo, hi), f=f, what="value range")
        some = got[5]["n"] > 0
        assert some.any() and (got[5]["min"][some] >= lo).all() and (got[5]["max"][some] <= hi).all()
        f.close()
        # the empty filter: every record empty, nothing decoded
        nobody = np.zeros(HAND_DOCS, dtype=bool)
        f = hand.s.filter(nobody)
        got = hand.check_g(entry, QUERIES, group_of, n_groups, x, values, col, mask=nobody, f=f, what="empty")
        assert got[4] == 0 and not got[3].any() and not got[6].any()
        assert got[5].tobytes() == GS.empty_records(len(QUERIES), n_groups).tobytes()
        f.close()


# ---- conservation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_the_groups_add_up_to_the_value_stats_entry(hand, maps, columns, entry):
    """every document grouped: per query the records' n and sum add up to the value-stats entry's, and their extremes are its"""
    for col_name in ("wide", "half", "top + 3"):
        values, col = columns[col_name]
        whole = hand.s.run_v(entry, QUERIES, col, edges_of(values, 0), None)[5]
        for map_name, n_groups in (("striped", 300), ("clustered", 256), ("long", 7)):
            group_of, x = maps.of(map_name, n_groups)
            assert (group_of[:HAND_DOCS] != FA.NONE).all()
            got = hand.run_g(entry, QUERIES, x, col, None)[5]
            assert np.array_equal(got["n"].sum(axis=1, dtype=np.uint64), whole["n"]), (col_name, map_name)
            assert np.array_equal(got["sum"].sum(axis=1, dtype=np.uint64), whole["sum"]), (col_name, map_name)
            assert np.array_equal(got["min"].min(axis=1), whole["min"]) and np.array_equal(got["max"].max(axis=1), whole["max"])


# ---- batches, passes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_batch_and_one_query_per_call(hand, maps, columns, entry):
    qs = _many_queries(300)
    assert [] in qs and len({tuple(q) for q in qs}) > 100
    values, col = columns["wide"]
    for name, n_groups in (("clustered", 7), ("striped", 300)):
        group_of, x = maps.of(name, n_groups)
        batch = hand.check_g(entry, qs, group_of, n_groups, x, values, col, what=("batch", name))
        for i, q in enumerate(qs):
            one = hand.run_g(entry, [q], x, col, None)
            _bit_equal([a[0] for a in one[:4] + one[5:]], [a[i] for a in batch[:4] + batch[5:]], (entry, name, i))


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, hand, maps, columns, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: the records of the queries of later passes lie at their own offset (the
    pass's first query), and every pass adds to a workspace that was sent once."""
    qs = _many_queries(60, seed=9) + QUERIES
    device.set_option("query_or_pass_pages", pass_pages)
    f = hand.s.filter(CLUSTERED)
    values, col = columns["wide"]
    for name, n_groups in (("clustered", 2), ("runs of 5", 257)):
        group_of, x = maps.of(name, n_groups)
        for entry in ENTRIES:
            got = hand.check_g(entry, qs, group_of, n_groups, x, values, col, what=name)
            back = hand.run_g(entry, qs[::-1], x, col, None)
            _bit_equal([a[::-1] for a in back[5:]], got[5:], (entry, name, "reversed"))
            hand.check_g(entry, qs, group_of, n_groups, x, values, col, mask=CLUSTERED, f=f, what=(name, "clustered"))
        assert int(got[5]["n"][len(qs) // 2:].sum()) > 0  # (queries of later passes match something)
    f.close()


# ---- null optional outputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_null_optional_outputs(device, hand, maps, columns, entry):
    values, col = columns["wide"]
    group_of, x = maps.of("clustered", 257)
    got = hand.check_g(entry, QUERIES, group_of, 257, x, values, col)
    terms, offs = device._pack_queries(QUERIES)
    n = len(QUERIES)
    fn = getattr(device._lib, f"dint_ranked_{entry}_group_stats_queries")
    for with_ids, with_rows, with_blocks in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        counts, matches = np.full(n, 77, dtype=np.uint64), np.full(n, 77, dtype=np.uint64)
        scores, docids = np.full((n, K), -1.0, dtype=np.float32), np.full((n, K), 77, dtype=np.uint32)
        recs, rows = np.full((n, 257), 77, dtype=GS.STATS_DTYPE), np.full((n, 257), 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        st = fn(hand.qi._h, hand.s.fd._h, hand.s.wand._h, K, terms.ctypes.data, offs.ctypes.data, None, x._h, col._h, n, counts.ctypes.data,
                matches.ctypes.data if with_ids else None, scores.ctypes.data, docids.ctypes.data if with_ids else None, recs.ctypes.data,
                rows.ctypes.data if with_rows else None, C.byref(blocks) if with_blocks else None, None)
        what = (entry, with_ids, with_rows, with_blocks)
        assert st == 0, what
        _bit_equal((counts, scores, recs), (got[0], got[1], got[5]), what)
        assert (docids.tobytes() == got[2].tobytes() and matches.tobytes() == got[3].tobytes()) if with_ids else ((docids == 77).all() and (matches == 77).all())
        assert rows.tobytes() == got[6].tobytes() if with_rows else (rows == 77).all()
        assert blocks.value == (got[4] if with_blocks else 77), what


# ---- errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, maps, columns, entry):
    call = getattr(device._lib, f"dint_ranked_{entry}_group_stats_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.s.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.s.ix.docs_dict), hand.s.ix.bytes, hand.s.ix.offsets)
    f_other = other.doc_filter(mask)
    values, col = columns["wide"]
    _, x = maps.of("clustered", 7)
    _, x_most = maps.of("clustered", 65536)

    def attempt(k, terms_, filt, x_, col_, null=(), offs_=offs, n=1):
        counts, matches = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
        scores, docids = np.full(1025, -1.0, dtype=np.float32), np.full(1025, 77, dtype=np.uint32)
        recs, rows = np.full(7, 77, dtype=GS.STATS_DTYPE), np.full(7, 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        st = call(hand.qi._h, hand.s.fd._h, hand.s.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  x_._h if x_ is not None else None, col_._h if col_ is not None else None, n,
                  None if "counts" in null else counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                  None if "recs" in null else recs.ctypes.data, rows.ctypes.data, C.byref(blocks), None)
        untouched = (counts[0] == 77 and matches[0] == 77 and (scores == -1.0).all() and (docids == 77).all() and (rows == 77).all()
                     and recs.tobytes() == np.full(7, 77, dtype=GS.STATS_DTYPE).tobytes() and blocks.value == 77)
        return st, untouched

    for filt in (None, f):
        assert attempt(0, terms, filt, x, col) == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, x, col) == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 6], dtype=np.uint32), filt, x, col) == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, x, col, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)  # decreasing offsets
        assert attempt(10, terms, filt, x, col, null=("counts",)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, None, col) == (DINT_ERR_ARG, True)  # no map
        assert attempt(10, terms, filt, x, None) == (DINT_ERR_ARG, True)  # no column
        assert attempt(10, terms, filt, x, col, null=("recs",)) == (DINT_ERR_ARG, True)
        # n_queries * n_groups just over 2^24: 257 queries of 65 536 groups, refused before any array is read (the arrays hold
        # one query: the sizes lie)
        assert attempt(10, terms, filt, x_most, col, n=(1 << 24) // 65536 + 1) == (DINT_ERR_ARG, True)
    assert attempt(10, terms, f_other, x, col) == (DINT_ERR_ARG, True)  # a filter of another query index
    if device.device_count() > 1:  # a map or a column on another device than the index (one device: these cases alone are left out)
        elsewhere = device.DocValues(1, values)
        assert attempt(10, terms, None, x, elsewhere) == (DINT_ERR_ARG, True)
        elsewhere.close()
        elsewhere = device.DocFacets(1, GS.named_maps(HAND_DOCS, 7)["clustered"], 7)
        assert attempt(10, terms, None, elsewhere, col) == (DINT_ERR_ARG, True)
        elsewhere.close()
    st, untouched = attempt(10, terms, f, x, col)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_g(entry, [[6]], x, col, f)
    with pytest.raises(device.DintError):
        hand.run_g(entry, [[0]], x, col, f_other)
    f_other.close()
    other.close()
    f.close()


# ---- beside the faceted and the value-stats calls -----------------------------------------------------------------------
def test_faceted_value_stats_and_group_stats_calls_in_turn(hand, maps, columns):
    """the three workspaces are separate: a faceted call, a value-stats call and a group-stats call in turn on one index, longer
    and shorter batches in between, leave every answer correct"""
    values, col = columns["wide"]
    group_of, x = maps.of("striped", 300)
    for entry in ENTRIES:
        hand.s.check_x(entry, QUERIES, group_of, 300, facets=x)
        hand.s.check_v(entry, QUERIES, values, col, edges_of(values, 257))
        hand.check_g(entry, QUERIES, group_of, 300, x, values, col)
        hand.s.check_x(entry, QUERIES[::-1], group_of, 300, facets=x)
        hand.check_g(entry, [[4], [], [0, 1]], group_of, 300, x, values, col)
        hand.s.check_v(entry, [[4], [], [0, 1]], values, col, edges_of(values, 1023))
        hand.check_g(entry, QUERIES[::-1], group_of, 300, x, values, col)
        hand.s.check_v(entry, QUERIES[::-1], values, col, edges_of(values, 1))
        hand.s.check_x(entry, [[4]], group_of, 300, facets=x)
        hand.check_g(entry, [[4]], group_of, 300, x, values, col)
