"""Exact percentiles on the GPU through the C ABI (dint_ranked_or_percentile_queries, dint_ranked_and_percentile_queries;
DESIGN.md 4d-percentiles): every query's count of valued matches and every requested percentile equal to the model's
(tests/percentiles.py: a sort), counts, scores, docids, matches and blocks_decoded equal to the filtered entry's on the same
arguments, byte for byte, and the statistics, where asked for, equal to the value-stats entry's with no edges. The index is the
hand-made one of tests/test_gpu_value_stats.py — 9 000 documents, a = 0 .. 2999, b = 5000 .. 8999, c = the evens, d = every
document (36 pages, the last one of 40 live slots), e = {10, 20, 30, 40}, and a sixth list that is empty. k = 10. Everything is
an integer: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import percentiles as PC
import value_stats as VS
from dint_amd import host
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import HAND_DOCS
from test_gpu_paging import CLUSTERED
from test_gpu_ranked_queries import _hand_made
from test_gpu_value_stats import EMPTY_LIST, QUERIES, Stats, _many_queries, _same

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")
M32 = 0xFFFFFFFF
K = 10
SETS = PC.percentile_sets(HAND_DOCS)


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


class Percentiles(Stats):
    """Stats (an index, its freqs dictionary and wand data on the device, the filtered and the value-stats entries and the
    model's matches) with the two percentile entries and their model."""

    def run_p(self, entry, qs, col, per_million, f, k=K, stats=True):
        """-> (counts, scores, docids, matches, blocks_decoded, value_counts, percentile_values, stats); without the stats no
        matches and blocks, and None for the records"""
        fn = self.qi.ranked_or_percentile_queries if entry == "or" else self.qi.ranked_and_percentile_queries
        return fn(self.fd, self.wand, qs, col, PC.percents(per_million), filter=f, k=k, with_stats=stats)

    def want_p(self, entry, qs, values, per_million, mask):
        return PC.stacked([PC.percentiles(self.matches_of(entry, q), mask, values, per_million) for q in qs], len(per_million))

    def check_p(self, entry, qs, values, col, per_million, k=K, mask=None, f=None, what=None):
        """the percentile call against the filtered entry on the same arguments — byte for byte, blocks_decoded too —, its counts
        and values against the model, its records against the value-stats entry's with no edges; twice: the two runs are
        byte-identical; and with a null stats: the same answers"""
        what = (entry, per_million, k, what)
        got = self.run_p(entry, qs, col, per_million, f, k)
        same = self.run_f(entry, qs, f, k)
        _bit_equal(got[:4], same[:4], what)
        assert got[4] == same[4], what
        assert got[6].shape == (len(qs), len(per_million)), what
        _bit_equal(got[5:7], self.want_p(entry, qs, values, per_million, mask), what)
        _bit_equal((got[7],), (self.run_v(entry, qs, col, [], f, k)[5],), what)
        assert got[5].tobytes() == got[7]["n"].tobytes(), what
        again = self.run_p(entry, qs, col, per_million, f, k)
        _bit_equal(again[:4] + again[5:], got[:4] + got[5:], what)
        assert again[4] == got[4], what
        bare = self.run_p(entry, qs, col, per_million, f, k, stats=False)
        assert len(bare) == 6 and bare[5] is None, what
        _bit_equal(bare[:5], got[:3] + got[5:7], what)
        return got


@pytest.fixture(scope="module")
def hand(device):
    """the hand-made index with one list more, which no block names, made as tests/test_gpu_value_stats.py makes it"""
    import ranked

    kind = host.MULTI_PACKED
    r = Percentiles(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
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
    return PC.named_columns(HAND_DOCS)


@pytest.fixture(scope="module")
def columns(device):
    cols = {name: (v, device.DocValues(0, v)) for name, v in hand_columns().items()}
    yield cols
    for _, c in cols.values():
        c.close()


# ---- the queries, the columns and the sets ------------------------------------------------------------------------------
def test_the_cases_are_what_they_are_said_to_be(hand):
    sizes = {e: [hand.matches_of(e, q)[1].size for q in QUERIES] for e in ENTRIES}
    for e in ENTRIES:
        assert [] in QUERIES and sizes[e][QUERIES.index([])] == 0 and sizes[e][QUERIES.index([EMPTY_LIST])] == 0
        assert sizes[e][QUERIES.index([3])] == HAND_DOCS and HAND_DOCS % 256 == 40  # 36 pages, the last one of 40 live slots
        assert sizes[e][QUERIES.index([4])] == 4 and any(s > 256 for s in sizes[e])
    assert [0, 0] in QUERIES and [2, 0, 2] in QUERIES and [0, 1] in QUERIES and [0] in QUERIES  # a repeated term; several; one
    assert set(SETS) == {"the minimum", "the maximum", "the median", "both ends", "descending, one twice", "sixteen, spread",
                         "sixteen, one prefix"}
    cols = hand_columns()
    every = hand.matches_of("or", [3])
    assert np.unique(PC.percentiles(every, None, cols["top byte"], SETS["sixteen, spread"])[1] >> 24).size == 16
    near = PC.percentiles(every, None, cols["v = d"], SETS["sixteen, one prefix"])[1]
    assert np.unique(near >> 8).size == 1 and np.unique(near).size == 16
    assert PC.percentiles(every, None, cols["two halves"], [500000])[1].tolist() == [PC.HALF_LOW]


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(hand_columns()))
def test_columns_and_percentile_sets(hand, columns, entry, name):
    values, col = columns[name]
    for sname, pm in SETS.items():
        got = hand.check_p(entry, QUERIES, values, col, pm, what=(name, sname))
        if name == "empty":
            assert not got[5].any() and not got[6].any()
    f = hand.filter(CLUSTERED)
    for sname in ("both ends", "sixteen, spread"):
        hand.check_p(entry, QUERIES, values, col, SETS[sname], mask=CLUSTERED, f=f, what=(name, sname, "clustered"))
    f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_query_with_one_valued_match(hand, device, entry):
    values = np.arange(11, dtype=np.uint32) * 0x01010101 + 5  # e = {10, 20, 30, 40}: only document 10 is below the column's end
    col = device.DocValues(0, values)
    for pm in SETS.values():
        got = hand.check_p(entry, QUERIES, values, col, pm, what="eleven documents")
        at = QUERIES.index([4])
        assert got[3][at] == 4 and got[5][at] == 1 and (got[6][at] == values[10]).all()
    col.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, columns, entry):
    values, col = columns["wide"]
    for k in (1, 1024):
        got = hand.check_p(entry, QUERIES, values, col, SETS["descending, one twice"], k=k)
    assert int(got[0].max()) == 1024 and int(got[5].max()) > 1024  # (the percentiles are over every match, not the top k)


# ---- filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_filters(hand, columns, entry):
    values, col = columns["v = d"]
    pm = SETS["sixteen, spread"]
    # a value-range filter from the same column: every percentile lies in [lo, hi]
    lo, hi = 2900, 5300
    f = hand.qi.doc_filter_from_values(col, lo, hi)
    got = hand.check_p(entry, QUERIES, values, col, pm, mask=DV.values_mask(values, lo, hi), f=f, what="value range")
    some = got[5] > 0
    assert some.any() and (got[6][some] >= lo).all() and (got[6][some] <= hi).all()
    f.close()
    # a bitmap filter, and under it a column shorter than the index
    other, ocol = columns["half"]
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    hand.check_p(entry, QUERIES, values, col, pm, mask=mask, f=f, what="a bitmap")
    hand.check_p(entry, QUERIES, other, ocol, pm, mask=mask, f=f, what="a bitmap, a short column")
    f.close()
    # the empty filter: no valued match, every percentile 0, nothing decoded
    nobody = np.zeros(HAND_DOCS, dtype=bool)
    f = hand.filter(nobody)
    got = hand.check_p(entry, QUERIES, values, col, pm, mask=nobody, f=f, what="empty")
    assert got[4] == 0 and not got[3].any() and not got[5].any() and not got[6].any()
    assert got[7].tobytes() == np.array([VS.EMPTY] * len(QUERIES), dtype=VS.STATS_DTYPE).tobytes()
    f.close()


# ---- batches, passes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_batch_and_one_query_per_call(hand, columns, entry):
    qs = _many_queries(300)
    assert [] in qs and len({tuple(q) for q in qs}) > 100
    for name, sname in (("wide", "sixteen, spread"), ("two halves", "the median")):
        values, col = columns[name]
        batch = hand.check_p(entry, qs, values, col, SETS[sname], what=("batch", name))
        for i, q in enumerate(qs):
            one = hand.run_p(entry, [q], col, SETS[sname], None)
            _same([x[0] for x in one[:4] + one[5:]], [x[i] for x in batch[:4] + batch[5:]], (entry, name, i))


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, hand, columns, pass_pages):
    """query_or_pass_pages cuts the OR call into passes: the rows, the states and the answers of the queries of later passes lie
    at their own offset (the pass's first query), and a query's four rounds complete within its pass."""
    qs = _many_queries(60, seed=9) + QUERIES
    device.set_option("query_or_pass_pages", pass_pages)
    f = hand.filter(CLUSTERED)
    for name, sname in (("wide", "descending, one twice"), ("v = d", "sixteen, one prefix")):
        values, col = columns[name]
        for entry in ENTRIES:
            got = hand.check_p(entry, qs, values, col, SETS[sname], what=name)
            back = hand.run_p(entry, qs[::-1], col, SETS[sname], None)
            _same([x[::-1] for x in back[5:]], got[5:], (entry, name, "reversed"))
            hand.check_p(entry, qs, values, col, SETS[sname], mask=CLUSTERED, f=f, what=(name, "clustered"))
        assert int(got[5][len(qs) // 2:].sum()) > 0  # (queries of later passes match something)
    f.close()


# ---- errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, columns, entry):
    call = getattr(device._lib, f"dint_ranked_{entry}_percentile_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    values, col = columns["v = d"]
    p3 = np.array([500000, 0, 1000000], dtype=np.uint32)

    def attempt(k, terms_, filt, col_, pm=p3, n_p=3, null=(), offs_=offs):
        counts, matches, vc = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
        scores, docids, pv = np.full(1025, -1.0, dtype=np.float32), np.full(1025, 77, dtype=np.uint32), np.full(32, 77, dtype=np.uint32)
        stats = np.full(1, 77, dtype=VS.STATS_DTYPE)
        blocks = C.c_uint64(77)
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                  col_._h if col_ is not None else None, pm.ctypes.data if pm is not None else None, n_p, 1,
                  None if "counts" in null else counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                  None if "vc" in null else vc.ctypes.data, None if "pv" in null else pv.ctypes.data,
                  None if "stats" in null else stats.ctypes.data, C.byref(blocks), None)
        untouched = (counts[0] == 77 and matches[0] == 77 and vc[0] == 77 and (scores == -1.0).all() and (docids == 77).all()
                     and (pv == 77).all() and stats.tobytes() == np.full(1, 77, dtype=VS.STATS_DTYPE).tobytes() and blocks.value == 77)
        return st, untouched

    for filt in (None, f):
        for null in ((), ("stats",)):
            assert attempt(0, terms, filt, col, null=null) == (DINT_ERR_ARG, True)
            assert attempt(1025, terms, filt, col, null=null) == (DINT_ERR_ARG, True)
            assert attempt(10, np.array([0, 6], dtype=np.uint32), filt, col, null=null) == (DINT_ERR_ARG, True)  # a term >= n_lists
            assert attempt(10, terms, filt, col, offs_=np.array([2, 0], dtype=np.uint64), null=null) == (DINT_ERR_ARG, True)  # decreasing offsets
            assert attempt(10, terms, filt, col, null=null + ("counts",)) == (DINT_ERR_ARG, True)
            assert attempt(10, terms, filt, None, null=null) == (DINT_ERR_ARG, True)  # no column
            assert attempt(10, terms, filt, col, null=null + ("vc",)) == (DINT_ERR_ARG, True)
            assert attempt(10, terms, filt, col, null=null + ("pv",)) == (DINT_ERR_ARG, True)
            assert attempt(10, terms, filt, col, pm=None, null=null) == (DINT_ERR_ARG, True)
            assert attempt(10, terms, filt, col, n_p=0, null=null) == (DINT_ERR_ARG, True)
            assert attempt(10, terms, filt, col, pm=np.zeros(17, dtype=np.uint32), n_p=17, null=null) == (DINT_ERR_ARG, True)
            assert attempt(10, terms, filt, col, pm=np.array([5, 1000001, 9], dtype=np.uint32), null=null) == (DINT_ERR_ARG, True)
    assert attempt(10, terms, f_other, col) == (DINT_ERR_ARG, True)  # a filter of another query index
    if device.device_count() > 1:  # a column on another device than the index (one device: this case alone is left out)
        elsewhere = device.DocValues(1, values)
        assert attempt(10, terms, None, elsewhere) == (DINT_ERR_ARG, True)
        elsewhere.close()
    # n_queries * n_percentiles past the cap: refused, though the offsets would hold
    n = (1 << 16) // 3 + 1
    many_offs = np.zeros(n + 1, dtype=np.uint64)
    counts, scores = np.full(n, 77, dtype=np.uint64), np.full(n * K, -1.0, dtype=np.float32)
    vc, pv = np.full(n, 77, dtype=np.uint64), np.full(3 * n, 77, dtype=np.uint32)
    assert call(hand.qi._h, hand.fd._h, hand.wand._h, K, None, many_offs.ctypes.data, None, col._h, p3.ctypes.data, 3, n, counts.ctypes.data, None,
                scores.ctypes.data, None, vc.ctypes.data, pv.ctypes.data, None, None, None) == DINT_ERR_ARG
    assert (counts == 77).all() and (vc == 77).all() and (pv == 77).all() and (scores == -1.0).all()
    # ... and one query fewer is taken: the largest call of three percentiles (every query empty)
    assert call(hand.qi._h, hand.fd._h, hand.wand._h, K, None, many_offs.ctypes.data, None, col._h, p3.ctypes.data, 3, n - 1, counts.ctypes.data, None,
                scores.ctypes.data, None, vc.ctypes.data, pv.ctypes.data, None, None, None) == 0
    assert not counts[:n - 1].any() and not vc[:n - 1].any() and not pv[:3 * (n - 1)].any() and vc[n - 1] == 77
    st, untouched = attempt(10, terms, f, col)
    assert st == 0 and not untouched
    with pytest.raises(device.DintError):
        hand.run_p(entry, [[6]], col, p3.tolist(), f)
    with pytest.raises(device.DintError):
        hand.run_p(entry, [[0]], col, p3.tolist(), f_other)
    for bad in ([], [-1], [100.5], list(range(17))):
        with pytest.raises(ValueError):
            (hand.qi.ranked_or_percentile_queries if entry == "or" else hand.qi.ranked_and_percentile_queries)(hand.fd, hand.wand, [[0]], col, bad)
    f_other.close()
    other.close()
    f.close()


# ---- beside the value-stats calls ---------------------------------------------------------------------------------------
def test_value_stats_and_percentile_calls_in_turn(hand, columns):
    """the workspaces are separate: a value-stats call, a percentile call and a value-stats call again on one index, longer and
    shorter batches and other percentile counts in between, leave every answer correct"""
    from test_gpu_value_stats import edges_of

    values, col = columns["wide"]
    for entry in ENTRIES:
        hand.check_v(entry, QUERIES, values, col, edges_of(values, 257))
        hand.check_p(entry, QUERIES, values, col, SETS["sixteen, spread"])
        hand.check_v(entry, QUERIES[::-1], values, col, edges_of(values, 16))
        hand.check_p(entry, [[4], [], [0, 1]], values, col, SETS["the median"])
        hand.check_p(entry, QUERIES[::-1], values, col, SETS["both ends"])
        hand.check_v(entry, [[4]], values, col, edges_of(values, 1))
        hand.check_p(entry, [[3]], values, col, SETS["sixteen, one prefix"])
