"""Document values on the GPU through the C ABI (dint_doc_values_create, dint_ranked_or_sorted_queries,
dint_ranked_and_sorted_queries, dint_doc_filter_create_from_values): counts, hit values, docIDs, BM25
scores, matches and skipped equal to the model's (tests/doc_values.py: the matches ordered by (value, docID), cut strictly
behind the cursor), bit for bit; matches and blocks_decoded equal to the filtered entry's; a value-range filter equal to the
bitmap filter of the same documents. The index is the hand-made one of the range, collapse and paging tests: 9 000 documents,
a document's lane is d & 63, norm_lens all 1. No tolerance anywhere."""
import ctypes as C
import threading

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import ranked
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_doc_filter import _bit_equal
from test_gpu_facets import HAND_DOCS
from test_gpu_paging import CLUSTERED, Paged
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import _hand_made
from test_gpu_ranked_range import HAND_QUERIES
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ENTRIES = ("or", "and")
ORDERS = (True, False)  # descending
KS = (1, 7, 256, 257, 1024)  # runs of 256, 512 and 1024 keys
M32 = 0xFFFFFFFF
SPIKES = [0, 63, 64, 255, 256, 8999]


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


class Sorted(Paged):
    """Paged (an index, its freqs dictionary and wand data on the device, the filtered and paged entries and the model's
    matches) with the two sorted entries and their model."""

    def run_s(self, entry, qs, col, desc, after, f, k, stats=True):
        """-> (counts, hit_values, docids, scores, matches, blocks_decoded, skipped); without the stats no matches and blocks"""
        fn = self.qi.ranked_or_sorted_queries if entry == "or" else self.qi.ranked_and_sorted_queries
        return fn(self.fd, self.wand, qs, col, descending=desc, after=after, filter=f, k=k, with_stats=stats)

    def want_s(self, entry, qs, values, desc, after, mask, k):
        after = after if after is not None else [None] * len(qs)
        return DV.stacked([DV.sorted_page(self.matches_of(entry, q), mask, values, desc, c, k) for q, c in zip(qs, after)], k)

    def check_s(self, entry, qs, values, col, desc, after, k=10, mask=None, f=None, what=None):
        """the sorted call against the model, bit for bit, and its matches and blocks_decoded against the filtered entry"""
        what = (entry, desc, k, what)
        got = self.run_s(entry, qs, col, desc, after, f, k)
        _bit_equal(got[:5] + got[6:], self.want_s(entry, qs, values, desc, after, mask, k), what)
        assert np.array_equal(got[0], np.minimum(got[4] - got[6], k)), what
        same = self.run_f(entry, qs, f, k)
        _bit_equal((got[4],), (same[3],), what)
        assert got[5] == same[4], what
        return got

    def ordered_s(self, entry, q, values, desc, mask=None):
        """the query's matches under the mask in the sorted order: (values, docids, scores)"""
        return DV.in_order(self.matches_of(entry, q), mask, values, desc)


@pytest.fixture(scope="module")
def hand(device):
    """test_gpu_ranked_range.py's hand-made index: a = 0 .. 2999, b = 5000 .. 8999, c = the evens, d = every doc (page j holds
    256 j .. 256 j + 255), e = {10, 20, 30, 40}; norm_lens all 1."""
    kind = host.MULTI_PACKED
    r = Sorted(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    yield r
    r.close()


def hand_columns():
    d = np.arange(HAND_DOCS, dtype=np.uint64)
    spikes = np.zeros(HAND_DOCS, dtype=np.uint32)
    spikes[SPIKES] = M32
    return {"constant": np.full(HAND_DOCS, 5, dtype=np.uint32), "v = d": d.astype(np.uint32), "lanes": (d & 63).astype(np.uint32),
            "reverse": (M32 - d).astype(np.uint32), "spikes": spikes, "all but the spikes": ~spikes,
            "short 1000": (d[:1000] * 7 % 1000 + 1).astype(np.uint32), "short 0": np.zeros(0, dtype=np.uint32)}


@pytest.fixture(scope="module")
def columns(device):
    cols = {name: (v, device.DocValues(0, v)) for name, v in hand_columns().items()}
    yield cols
    for _, c in cols.values():
        c.close()


def _filters(hand):
    return ((None, None), (CLUSTERED, hand.filter(CLUSTERED)))


# ---- the columns --------------------------------------------------------------------------------------------------------
def test_the_columns_are_what_they_are_said_to_be(hand):
    cols = hand_columns()
    every = hand.matches_of("or", [3])  # d: every document
    for desc in ORDERS:
        v, ids, _ = DV.in_order(every, None, cols["constant"], desc)
        assert np.array_equal(ids, np.arange(HAND_DOCS))  # constant: the docID's order
        v, ids, _ = DV.in_order(every, None, cols["lanes"], desc)
        assert v[6] == v[7] and v[9] == v[10] and (np.diff(ids[:100]) > 0).all()  # the cut of k = 7 and 10 inside a run of equal values
        n, hv, docids, _, m, _ = DV.sorted_page(every, None, cols["spikes"], desc, None, 7)
        assert (docids[:6].tolist() == SPIKES and hv[6] == 0) if desc else (hv[:7] == 0).all() and docids[:3].tolist() == [1, 2, 3]
        n, hv, docids, _, m, _ = DV.sorted_page(every, None, cols["all but the spikes"], desc, None, 7)
        assert (docids[:6].tolist() == SPIKES and hv[6] == M32) if not desc else (hv[:7] == M32).all()
        for name, n_col in (("short 1000", 1000), ("short 0", 0)):
            v, ids, _ = DV.in_order(every, None, cols[name], desc)
            assert (v[ids >= n_col] == 0).all() and (n_col == 0 or v[ids < n_col].min() > 0)
            missing = ids[n_col:] if desc else ids[:HAND_DOCS - n_col]  # value 0: the last descending, the first ascending
            assert np.array_equal(missing, np.arange(n_col, HAND_DOCS))  # ... and among themselves by docID
    v, ids, _ = DV.in_order(every, None, cols["v = d"], True)
    assert ids[:3].tolist() == [8999, 8998, 8997]  # descending: the best keys lie in the LAST pages and runs
    v, ids, _ = DV.in_order(every, None, cols["reverse"], False)
    assert ids[:3].tolist() == [8999, 8998, 8997] and v[0] == M32 - 8999
    for k, R in zip(KS, (256, 256, 256, 512, 1024)):
        assert max(256, 1 << (k - 1).bit_length()) == R
    sizes = {e: [hand.matches_of(e, q)[1].size for q in HAND_QUERIES] for e in ENTRIES}
    for e in ENTRIES:  # queries with more than k matches, with fewer, with none, and an empty one inside the batch
        assert max(sizes[e]) > 1024 and any(0 < s < 7 for s in sizes[e]) and [] in HAND_QUERIES[:-1]
    assert 0 in sizes["and"] and sizes["and"][HAND_QUERIES.index([0, 1])] == 0


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(hand_columns()))
def test_columns_orders_and_k(hand, columns, entry, name):
    values, col = columns[name]
    for mask, f in _filters(hand):
        for desc in ORDERS:
            for k in KS:
                hand.check_s(entry, HAND_QUERIES, values, col, desc, None, k=k, mask=mask, f=f, what=name)
        if f is not None:
            f.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_scores_are_the_filtered_entrys_and_nullable(device, hand, columns, entry):
    values, col = columns["lanes"]
    for mask, f in _filters(hand):
        k = 1024
        got = hand.run_s(entry, HAND_QUERIES, col, True, None, f, k)
        want = {(qi, int(d)): s for qi, q in enumerate(HAND_QUERIES) for s, d in zip(*DF.top_in_filter(
            hand.matches_of(entry, q), mask if mask is not None else np.ones(HAND_DOCS, dtype=bool), HAND_DOCS)[1:3])}
        for qi in range(len(HAND_QUERIES)):
            for i in range(int(got[0][qi])):
                assert got[3][qi, i].tobytes() == np.float32(want[(qi, int(got[2][qi, i]))]).tobytes()
        # scores null: the other outputs unchanged
        terms, offs = device._pack_queries(HAND_QUERIES)
        n = len(HAND_QUERIES)
        counts, matches, skipped = (np.full(n, 77, dtype=np.uint64) for _ in range(3))
        hv, docids = np.full((n, k), 77, dtype=np.uint32), np.full((n, k), 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        fn = getattr(device._lib, f"dint_ranked_{entry}_sorted_queries")
        st = fn(hand.qi._h, hand.fd._h, hand.wand._h, k, terms.ctypes.data, offs.ctypes.data, f._h if f is not None else None, col._h, 0, None,
                n, counts.ctypes.data, matches.ctypes.data, skipped.ctypes.data, hv.ctypes.data, docids.ctypes.data, None, C.byref(blocks), None)
        assert st == 0
        _bit_equal((counts, hv, docids, matches, skipped), (got[0], got[1], got[2], got[4], got[6]), entry)
        assert blocks.value == got[5]
        # ... and with only the required outputs, under unset cursors that carry a value and a docID: from the start all the same
        counts2, docids2 = np.full(n, 77, dtype=np.uint64), np.full((n, k), 77, dtype=np.uint32)
        unset = np.zeros(n, dtype=device._VALUE_CURSOR)
        unset["value"], unset["docid"] = M32 - np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32) * 1000
        st = fn(hand.qi._h, hand.fd._h, hand.wand._h, k, terms.ctypes.data, offs.ctypes.data, f._h if f is not None else None, col._h, 0,
                unset.ctypes.data, n, counts2.ctypes.data, None, None, None, docids2.ctypes.data, None, None, None)
        assert st == 0
        _bit_equal((counts2, docids2), (got[0], got[2]), entry)
        if f is not None:
            f.close()


# ---- cursors ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_cursor_edges(hand, columns, entry):
    dropped = {True: 0, False: 0}  # per order: the queries whose first match the all-ones key dropped
    for name in ("lanes", "v = d", "spikes"):
        values, col = columns[name]
        for mask, f in _filters(hand):
            for desc in ORDERS:
                firsts = [hand.ordered_s(entry, q, values, desc, mask) for q in HAND_QUERIES]
                at = lambda i: [((int(v[i]), int(ids[i])) if ids.size else None) for v, ids, _ in firsts]  # noqa: E731
                got = hand.check_s(entry, HAND_QUERIES, values, col, desc, at(0), mask=mask, f=f, what="the first match")
                assert np.array_equal(got[6], (got[4] > 0).astype(np.uint64))
                got = hand.check_s(entry, HAND_QUERIES, values, col, desc, at(-1), mask=mask, f=f, what="the last match")
                assert not got[0].any() and np.array_equal(got[6], got[4]) and got[4].sum() > 1000
                assert (got[2] == M32).all() and not got[1].any() and not got[3].any()
                start = hand.check_s(entry, HAND_QUERIES, values, col, desc, None, mask=mask, f=f, what="from the start")
                got = hand.check_s(entry, HAND_QUERIES, values, col, desc, [None] * len(HAND_QUERIES), mask=mask, f=f, what="unset cursors")
                _bit_equal(got[:5] + got[6:], start[:5] + start[6:], name)
                assert not got[6].any()
                # the two "all-ones key" cursors: (0xFFFFFFFF, 0) descending and (0, 0) ascending drop exactly document 0, and only
                # where it is a match with that value
                ones = (M32, 0) if desc else (0, 0)
                got = hand.check_s(entry, HAND_QUERIES, values, col, desc, [ones] * len(HAND_QUERIES), mask=mask, f=f, what="the all-ones key")
                drops = [int(ids.size and ids[0] == 0 and v[0] == ones[0]) for v, ids, _ in firsts]
                assert got[6].tolist() == drops
                dropped[desc] += sum(drops)
            if f is not None:
                f.close()
    assert dropped[True] >= 2 and dropped[False] >= 2


@pytest.mark.parametrize("entry", ENTRIES)
def test_cursors_inside_a_run_of_equal_values(hand, columns, entry):
    """Under the lanes column a value's run is a lane's documents, ascending. The cursor at a match inside the run, at a docID
    that is no match between two matched ones, at docID 0 and 0xFFFFFFFF, and at the values next to the run's."""
    values, col = columns["lanes"]
    for mask, f in _filters(hand):
        for desc in ORDERS:
            for q in ([3], [2, 3], [0, 1], [2, 0, 2]):
                v, ids, _ = hand.ordered_s(entry, q, values, desc, mask)
                if ids.size < 3:
                    continue
                x = int(v[ids.size // 2])
                run = ids[v == x]
                assert run.size >= 3 and (np.diff(run.astype(np.int64)) > 1).all()
                inside = int(run[run.size // 2])
                cursors = [(x, inside), (x, inside + 1), (x, 0), (x, M32), (x, int(run[0])), (x, int(run[-1])), (x + 1, 0), (x - 1, M32)]
                for k in (10, 300):
                    got = hand.check_s(entry, [q] * len(cursors), values, col, desc, cursors, k=k, mask=mask, f=f, what=q)
                before, through = int((v > x).sum() if desc else (v < x).sum()), int((v >= x).sum() if desc else (v <= x).sum())
                assert got[6][0] == got[6][1] == before + run.size // 2 + 1  # the gap after a match cuts where the match does
                assert got[6][2] == before + (1 if run[0] == 0 else 0) and got[6][3] == through and got[6][5] == through
        if f is not None:
            f.close()


def _cut_cases(desc):
    """cursors whose cut falls where the kernel's waves and pages meet, under [3] and v = d ascending / reverse descending
    (the order is the docID's, a slot per document) and, under OR [0, 1], between the pages of two terms"""
    val = (lambda d: M32 - d) if desc else (lambda d: d)
    cases = {"lanes 62 | 63": ([3], (val(318), 318)), "lanes 63 | 64": ([3], (val(319), 319)), "a page's last slot": ([3], (val(511), 511)),
             "the index's last slot": ([3], (val(8999), 8999)), "lane 0 | 1": ([3], (val(0), 0)),
             "between the pages of two terms": ([0, 1], (val(2999), 2999))}
    return cases


@pytest.mark.parametrize("entry", ENTRIES)
def test_cuts_at_slot_boundaries(hand, columns, entry):
    for desc in ORDERS:
        values, col = columns["reverse" if desc else "v = d"]
        cases = _cut_cases(desc)
        v, ids, _ = hand.ordered_s("or", [3], values, desc)
        assert np.array_equal(ids, np.arange(HAND_DOCS))
        for name, d in (("lanes 62 | 63", 318), ("lanes 63 | 64", 319), ("a page's last slot", 511)):
            n, _, docids, _, m, skipped = DV.sorted_page(hand.matches_of("or", [3]), None, values, desc, cases[name][1], 2)
            assert skipped == d + 1 and docids.tolist() == [d + 1, d + 2] and m == 9000
        n, _, docids, _, m, skipped = DV.sorted_page(hand.matches_of("or", [0, 1]), None, values, desc, cases["between the pages of two terms"][1], 3)
        assert skipped == 3000 and docids.tolist() == [5000, 5001, 5002] and m == 7000
        qs, after = [q for q, _ in cases.values()], [c for _, c in cases.values()]
        for k in (1, 2, 300):
            hand.check_s(entry, qs, values, col, desc, after, k=k, what="cuts")
        for q, c in zip(qs, after):  # ... and a query per call
            hand.check_s(entry, [q], values, col, desc, [c], k=5, what=c)


# ---- walks --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_walks_through_ranked_pages(hand, columns, entry):
    deep = [q for q in HAND_QUERIES if hand.matches_of(entry, q)[1].size > 1024]
    assert len(deep) >= 3
    f = hand.filter(CLUSTERED)
    few = min((q for q in HAND_QUERIES if hand.ordered_s(entry, q, columns["lanes"][0], True, CLUSTERED)[1].size > 100),
              key=lambda q: hand.ordered_s(entry, q, columns["lanes"][0], True, CLUSTERED)[1].size)
    smallest = min(deep, key=lambda q: hand.matches_of(entry, q)[1].size)
    most = max(deep, key=lambda q: hand.ordered_s(entry, q, columns["lanes"][0], True, CLUSTERED)[1].size)
    assert hand.ordered_s(entry, most, columns["lanes"][0], True, CLUSTERED)[1].size > 1024
    for name, desc, k, qs, mask, filt in (("lanes", True, 1024, deep[:3] + [[4], []], None, None), ("spikes", False, 64, [smallest], None, None),
                                          ("lanes", False, 7, [few], CLUSTERED, f), ("short 1000", True, 1024, [most, [4]], CLUSTERED, f)):
        values, col = columns[name]
        seen = {i: ([], [], []) for i in range(len(qs))}
        n_pages = 0
        for ids, counts, hv, docids, scores, skipped in hand.qi.ranked_pages(entry + "_sorted", hand.fd, hand.wand, qs, k=k, filter=filt,
                                                                             values=col, descending=desc):
            n_pages += 1
            for j, i in enumerate(ids.tolist()):
                assert int(skipped[j]) == len(seen[i][1])  # skipped: the hits before
                n = int(counts[j])
                seen[i][0].extend(hv[j][:n].tolist()), seen[i][1].extend(docids[j][:n].tolist()), seen[i][2].append(scores[j][:n])
        assert n_pages >= 2
        for i, q in enumerate(qs):
            v, d, sc = hand.ordered_s(entry, q, values, desc, mask)
            assert seen[i][0] == v.tolist() and seen[i][1] == d.tolist(), (entry, name, q)
            assert np.concatenate(seen[i][2] + [np.zeros(0, np.float32)]).tobytes() == sc.tobytes(), (entry, name, q)
    assert len(list(hand.qi.ranked_pages(entry + "_sorted", hand.fd, hand.wand, deep, k=7, values=columns["lanes"][1], max_pages=1))) == 1
    with pytest.raises(ValueError):
        list(hand.qi.ranked_pages(entry + "_sorted", hand.fd, hand.wand, deep, k=7))
    f.close()


# ---- batches, passes, call sequences ------------------------------------------------------------------------------------
@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_batch_of_cursors_in_many_passes(device, small_corpus, pass_pages):
    """a different cursor per query and some None, an empty query inside the batch, two queries with equal terms and different
    cursors; query_or_pass_pages cuts the OR call into passes, and a later pass's counters and hit scores lie at the pass's
    query offset. Behind the sorted call an unsorted ranked call and a paged call give their own answers; two calls in a row."""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Sorted(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:40] + heavy_queries(ix.lens, 8, seed=2) + [[], [0]]
    qs = qs + [qs[-3], qs[0]]  # equal terms, other cursors
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    rng = np.random.default_rng(11)
    values = rng.integers(0, 40, r.num_docs).astype(np.uint32)
    col = device.DocValues(0, values)
    device.set_option("query_or_pass_pages", pass_pages)
    for entry in ENTRIES:
        for m, filt in ((None, None), (mask, f)):
            desc = bool(rng.integers(0, 2))
            after = []
            for q in qs:
                v, ids, _ = r.ordered_s(entry, q, values, desc, m)
                after.append(DV.draw_cursor(rng, v, ids, r.num_docs) if ids.size else None)
            got = r.check_s(entry, qs, values, col, desc, after, mask=m, f=filt, what=pass_pages)
            assert int(got[6][len(qs) // 2:].sum()) > 0 and got[6][-4] == 0 and got[4][-4] == 0
            back = r.run_s(entry, qs[::-1], col, desc, after[::-1], filt, 10)
            for j in (0, 1, 2, 3, 4, 6):
                assert np.asarray(back[j][::-1]).tobytes() == np.asarray(got[j]).tobytes(), (entry, j)
            # an unsorted ranked call and a paged call behind a sorted one: their own answers
            same = r.run_f(entry, qs, filt, 10)
            _bit_equal(same[:4], r.want_f(entry, qs, m if m is not None else np.ones(r.num_docs, dtype=bool), 10), entry)
            r.check_p(entry, qs[:9], [None] * 9, mask=m, f=filt, what="a paged call behind a sorted one")
            r.check_s(entry, qs[:5], values, col, not desc, after[5:10], mask=m, f=filt, what="a shorter batch behind a longer one")
    col.close()
    f.close()
    r.close()


def test_two_threads_one_index_one_column(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Sorted(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:60] + heavy_queries(ix.lens, 6)
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None)
    f = r.filter(mask)
    values = (np.arange(r.num_docs, dtype=np.uint64) * 2654435761 % 97).astype(np.uint32)
    col = device.DocValues(0, values)
    masks = {"or": None, "and": mask}
    after = {e: [DV.last_hit(*DV.sorted_page(r.matches_of(e, q), masks[e], values, e == "or", None, 4)[:3]) for q in qs] for e in ENTRIES}
    want = {e: r.want_s(e, qs, values, e == "or", after[e], masks[e], 10) for e in ENTRIES}
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine = ENTRIES[which]
            for _ in range(3):
                got = r.run_s(mine, qs, col, mine == "or", after[mine], f if mine == "and" else None, 10)
                _bit_equal(got[:5] + got[6:], want[mine])
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    col.close()
    f.close()
    r.close()


# ---- errors -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, columns, entry):
    lib = device._lib
    fn = getattr(lib, f"dint_ranked_{entry}_sorted_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)
    col = columns["lanes"][1]
    good = np.array([(3, 3, 1)], dtype=device._VALUE_CURSOR)

    def attempt(k, terms_, filt, cursor, null=(), offs_=offs, values=col, order=0):
        out = {"counts": np.full(1, 77, dtype=np.uint64), "matches": np.full(1, 77, dtype=np.uint64), "skipped": np.full(1, 77, dtype=np.uint64),
               "hit_values": np.full(1025, 77, dtype=np.uint32), "docids": np.full(1025, 77, dtype=np.uint32),
               "scores": np.full(1025, -1.0, dtype=np.float32)}
        blocks = C.c_uint64(77)
        p = {name: None if name in null else a.ctypes.data for name, a in out.items()}
        st = fn(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs_.ctypes.data, filt._h if filt is not None else None,
                values._h if values is not None else None, order, cursor.ctypes.data if cursor is not None else None, 1, p["counts"],
                p["matches"], p["skipped"], p["hit_values"], p["docids"], p["scores"], C.byref(blocks), None)
        untouched = all((a == (-1.0 if name == "scores" else 77)).all() for name, a in out.items()) and blocks.value == 77
        return st, untouched

    for filt in (None, f):
        assert attempt(0, terms, filt, good) == (DINT_ERR_ARG, True)
        assert attempt(1025, terms, filt, good) == (DINT_ERR_ARG, True)
        assert attempt(10, np.array([0, 5], dtype=np.uint32), filt, good) == (DINT_ERR_ARG, True)  # a term >= n_lists
        assert attempt(10, terms, filt, good, offs_=np.array([2, 0], dtype=np.uint64)) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, good, values=None) == (DINT_ERR_ARG, True)  # no column
        assert attempt(10, terms, filt, good, order=2) == (DINT_ERR_ARG, True)
        assert attempt(10, terms, filt, good, order=M32) == (DINT_ERR_ARG, True)
        for name in ("counts", "docids"):
            assert attempt(10, terms, filt, good, null=(name,)) == (DINT_ERR_ARG, True), name
    assert attempt(10, terms, f_other, good) == (DINT_ERR_ARG, True)  # a filter of another query index
    st, untouched = attempt(10, terms, f, good)
    assert st == 0 and not untouched
    assert attempt(10, terms, f, good, null=("matches", "skipped", "hit_values", "scores"))[0] == 0  # the nullable outputs
    assert attempt(10, terms, f, None)[0] == 0 and attempt(10, terms, f, good, order=1)[0] == 0
    # the handle and the value-range filter
    h = C.c_void_p(77)
    v = np.zeros(4, dtype=np.uint32)
    assert lib.dint_doc_values_create(0, v.ctypes.data, 1 << 32, C.byref(h)) == DINT_ERR_ARG and h.value is None
    assert lib.dint_doc_values_create(0, None, 4, C.byref(h)) == DINT_ERR_ARG and lib.dint_doc_values_create(0, v.ctypes.data, 4, None) == DINT_ERR_ARG
    assert lib.dint_doc_filter_create_from_values(None, col._h, 0, 1, C.byref(h)) == DINT_ERR_ARG
    assert lib.dint_doc_filter_create_from_values(hand.qi._h, None, 0, 1, C.byref(h)) == DINT_ERR_ARG
    assert lib.dint_doc_filter_create_from_values(hand.qi._h, col._h, 0, 1, None) == DINT_ERR_ARG
    empty = device.DocValues(0, np.zeros(0, dtype=np.uint32))
    assert empty.num_docs == 0 and col.num_docs == HAND_DOCS
    empty.close()
    f_other.close()
    other.close()
    f.close()


# ---- docIDs at the top of the u32 range ---------------------------------------------------------------------------------
def test_docids_near_2_to_the_32_under_a_short_column(device):
    """docIDs up to 0xFFFFFFFE under a column of 1 000 documents (a full one would be 16 GB): the high documents have value 0
    and go by docID; 0xFFFFFFFF - d does not wrap for them"""
    kind = host.SINGLE_PACKED
    lists = [np.arange(TOP - 599, TOP + 1, dtype=np.uint64).astype(np.uint32), np.array([0, 5, TOP], dtype=np.uint32),
             np.concatenate([np.arange(0, 300, 3, dtype=np.uint64), np.arange(TOP - 298, TOP + 1, 2, dtype=np.uint64)]).astype(np.uint32)]
    rng = np.random.default_rng(5)
    freqs = [rng.integers(1, 3, x.size).astype(np.uint32) for x in lists]
    h = HighIndex(device, kind, lists, freqs)
    num_docs = TOP + 1
    nl = np.zeros(num_docs, dtype=np.float32)
    nl[h.docids] = 1.0
    qi, wand = device.QueryIndex(h.dd, h.index, h.offsets), device.WandData(nl)
    bl = ranked.BuilderLists(h.docids, h.freqs, h.bounds)
    values = (np.arange(1000, dtype=np.uint64) % 7 + 1).astype(np.uint32)
    col = device.DocValues(0, values)
    qs = [[0], [1], [0, 1], [0, 2], [1, 2], [0, 1, 2], []]
    for entry, fn in (("or", qi.ranked_or_sorted_queries), ("and", qi.ranked_and_sorted_queries)):
        every = [DF.every_match(bl, q, nl, num_docs, entry == "and") for q in qs]
        for desc in ORDERS:
            for pick in (None, 0, -1, 1):
                after = []
                for m in every:
                    v, ids, _ = DV.in_order(m, None, values, desc)
                    after.append((int(v[min(pick, ids.size - 1)]), int(ids[min(pick, ids.size - 1)])) if ids.size and pick is not None else None)
                if pick == 0:
                    after[0] = (0, TOP)  # the largest docID, value 0
                if pick == 1:
                    after[0] = (0, M32)  # past every docID
                got = fn(h.fd, wand, qs, col, descending=desc, after=after, k=10, with_stats=True)
                _bit_equal(got[:5] + got[6:], DV.stacked([DV.sorted_page(m, None, values, desc, c, 10) for m, c in zip(every, after)], 10),
                           (entry, desc, pick))
    col.close()
    qi.close()
    wand.close()


# ---- doc_filter_from_values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_col", [0, 1, 63, 64, 65, 8999])
def test_a_value_range_filter_is_the_bitmap_filter(device, hand, n_col):
    """columns that end in the last word, a lone word, at a word boundary; intervals: everything, lo == hi, lo > hi, one that
    matches nothing. The info and every filtered and sorted answer equal the host-built bitmap's."""
    rng = np.random.default_rng(n_col)
    values = rng.integers(0, 5, n_col).astype(np.uint32)
    if n_col:
        values[-1] = 3  # (the last document, the last bit of the last word)
    if n_col > 1:
        values[0] = M32
    col = device.DocValues(0, values)
    sort_values, sort_col = hand_columns()["lanes"], None
    sort_col = device.DocValues(0, sort_values)
    for lo, hi in ((0, M32), (3, 3), (4, 2), (7, 1000), (1, M32), (M32, M32), (0, 0)):
        mask = DV.values_mask(values, lo, hi)
        assert mask.size == n_col and (lo <= hi or not mask.any()) and ((lo, hi) != (7, 1000) or not mask.any())
        assert (lo, hi) != (0, M32) or mask.all()
        f1, f2 = hand.qi.doc_filter(mask), hand.qi.doc_filter_from_values(col, lo, hi)
        i1, i2 = f1.info, f2.info
        assert (i2.num_docs, i2.n_set, i2.n_blocks, i2.live_blocks) == (i1.num_docs, i1.n_set, i1.n_blocks, i1.live_blocks) and i2.n_set == mask.sum()
        assert i2.num_docs == n_col
        for entry in ENTRIES:
            for k in (10, 1024):
                a, b = hand.run_f(entry, HAND_QUERIES, f1, k), hand.run_f(entry, HAND_QUERIES, f2, k)
                _bit_equal(b[:4], a[:4], (entry, lo, hi))
                assert a[4] == b[4]
            _bit_equal(b[:4], hand.want_f(entry, HAND_QUERIES, mask, 1024), (entry, lo, hi))
            a = hand.check_s(entry, HAND_QUERIES, sort_values, sort_col, False, None, mask=mask, f=f1, what=(lo, hi))
            b = hand.run_s(entry, HAND_QUERIES, sort_col, False, None, f2, 10)
            _bit_equal(b, a, (entry, lo, hi))
        f1.close()
        f2.close()
    sort_col.close()
    col.close()


def test_from_float32_sorts_as_the_floats(device, hand):
    x = np.random.default_rng(3).normal(size=HAND_DOCS).astype(np.float32)
    x[[5, 6]] = (0.0, -0.0)
    col = device.DocValues.from_float32(0, x)
    keys = device.DocValues.float32_keys(x)
    got = hand.check_s("or", [[3]], keys, col, True, None, k=1024)
    assert (np.diff(x[got[2][0]]) <= 0).all()
    with pytest.raises(ValueError):
        device.DocValues.from_float32(0, np.array([1.0, np.nan], dtype=np.float32))
    col.close()
