"""DocID-range ranked queries on the GPU through the C ABI (dint_ranked_or_range_queries, dint_ranked_and_range_queries;
DESIGN.md 4d-range): counts, BM25 scores, docIDs and match counts bit-equal to the model (tests/ranked_range.py: the
unranged models filtered to the range), blocks_decoded equal to the blocks in range of the host block table, and the
unrestricted range equal to the unranged entries' own output."""
import ctypes as C
import threading

import numpy as np
import pytest

import ranked
import ranked_range as RR
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import Ranked, _assert_equal, _hand_made
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
ALL = (0, 0xFFFFFFFF)
KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]
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


def _same_row(one, got, i):
    """row 0 of a one-query call's (counts, scores, docids, matches) is row i of the batch's, bit for bit"""
    return all(np.asarray(one[j][0]).tobytes() == np.asarray(got[j][i]).tobytes() for j in range(4))


class Ranged(Ranked):
    """Ranked (an index, its freqs dictionary and wand data on the device) with the two ranged entries and their model.
    every: {(entry, query)} -> every match of the unranged model, computed once."""

    def __init__(self, device, ix, kind, num_docs=None, norm_lens=None, every=None):
        super().__init__(device, ix, kind, num_docs=num_docs)
        if norm_lens is not None:
            self.wand.close()
            self.norm_lens, self.wand = norm_lens, device.WandData(norm_lens)
        self.every = every if every is not None else {}
        self.blocks = self.qi.blocks

    def run(self, entry, qs, ranges, k, stats=True):
        fn = self.qi.ranked_or_range_queries if entry == "or" else self.qi.ranked_and_range_queries
        return fn(self.fd, self.wand, qs, ranges, k=k, with_stats=stats)

    def unranged(self, entry, qs, k):
        return (self.qi.ranked_or_queries if entry == "or" else self.qi.ranked_and_queries)(self.fd, self.wand, qs, k=k)

    def matches_of(self, entry, q):
        key = (entry, tuple(int(t) for t in q))
        if key not in self.every:
            self.every[key] = RR.every_match(self.lists, q, self.norm_lens, self.num_docs, entry == "and")
        return self.every[key]

    def want(self, entry, qs, ranges, k):
        """-> (counts, scores, docids, matches) of the model"""
        if ranges is None:
            ranges = [ALL] * len(qs)
        out = [RR.top_in_range(self.matches_of(entry, q), int(lo), int(hi), k) for q, (lo, hi) in zip(qs, np.asarray(ranges).tolist())]
        return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]) if out else np.zeros((0, k), np.float32),
                np.stack([o[2] for o in out]) if out else np.zeros((0, k), np.uint32), np.array([o[3] for o in out], dtype=np.uint64))

    def want_blocks(self, entry, qs, ranges):
        """OR: every distinct term's blocks in range; AND: the rarest list's (shortest, equal lengths by term id)"""
        if ranges is None:
            ranges = [ALL] * len(qs)
        total = 0
        for q, (lo, hi) in zip(qs, np.asarray(ranges).tolist()):
            terms = sorted(set(int(t) for t in q))
            if entry == "and" and terms:
                terms = [min(terms, key=lambda t: (int(self.ix.lens[t]), t))]
            total += sum(RR.n_blocks_in_range(self.blocks, t, int(lo), int(hi)) for t in terms)
        return total

    def check(self, entry, qs, ranges, k, what=None):
        got = self.run(entry, qs, ranges, k)
        want = self.want(entry, qs, ranges, k)
        for g, w in zip(got[:4], want):
            if g.dtype == np.float32:
                assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (entry, k, what)  # bit-equal scores
            else:
                assert np.array_equal(g, w), (entry, k, what)
        assert np.array_equal(got[0], np.minimum(got[3], k))
        assert got[4] == self.want_blocks(entry, qs, ranges), (entry, k, what)
        return got


# ---- the hand-made index: block edges at known docIDs -------------------------------------------------------------
# lists: a = 0 .. 2999 (blocks [256 j, 256 j + 255], the last one 2816 .. 2999), b = 5000 .. 8999 (blocks from 5000 + 256 j,
# the last one 8840 .. 8999), c = the evens (blocks [512 j, 512 j + 510]), d = every doc, e = {10, 20, 30, 40}
HAND_QUERIES = [[0, 1], [1, 0], [3], [3, 4], [2, 4], [0, 2], [4], [2, 3, 4], [0, 1, 4], [0], [1], [0, 0], [2, 0, 2], [], [1, 2, 3]]
HAND_RANGES = {
    "inside one block": (300, 400),
    "lo a block's max": (255, 600),
    "lo a block's max + 1": (256, 600),
    "hi - 1 a block's max": (100, 256),          # (a's, d's; hi is the next block's base)
    "hi - 1 a block's max and hi the next one's base (c)": (100, 511),
    "hi the next block's first docID (c)": (100, 512),   # (its base is 511: in range, and nothing of it is)
    "hi past the next block's first docID (c)": (100, 513),
    "hi b's first base": (4000, 5000),
    "hi b's first docID + 1": (4000, 5001),
    "ends in a's short last block": (2700, 2900),
    "ends in b's and d's short last block": (8700, 8950),
    "one docID": (2816, 2817),
    "wholly before b": (10, 50),
    "wholly after a": (6000, 6100),
    "after everything": (9000, 10000),
    "the gap between a and b": (3000, 5000),
    "inside the gap": (3500, 3600),
    "lo == hi": (500, 500),
    "lo > hi": (600, 500),
    "lo > hi at the ends": (0xFFFFFFFF, 0),
    "everything": ALL,
    "the whole space": (0, 9000),
}


@pytest.fixture(scope="module")
def hand(device):
    kind = host.MULTI_PACKED
    r = Ranged(device, _hand_made(device, kind), kind, num_docs=9000, norm_lens=np.ones(9000, dtype=np.float32))
    yield r
    r.close()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(HAND_RANGES))
def test_block_boundaries(hand, entry, name):
    lo, hi = HAND_RANGES[name]
    ranges = [(lo, hi)] * len(HAND_QUERIES)
    for k in (10, 1000):
        got = hand.check(entry, HAND_QUERIES, ranges, k, name)
    if lo >= hi or name == "after everything":
        assert got[4] == 0 and not got[0].any() and not got[3].any()  # decodes nothing, selects nothing
    # one query per call: the same rows
    for i in (0, 4, 8, 11):
        one = hand.check(entry, [HAND_QUERIES[i]], [ranges[i]], 1000, (name, i))
        assert _same_row(one, got, i)


def test_boundary_cases_are_what_they_are_said_to_be(hand):
    """The block table's maxima put the named ranges on the edges, and the gap and one-sided cases decode what they must."""
    maxima = lambda t: hand.blocks["max"][hand.blocks["list"] == t].tolist()  # noqa: E731
    assert maxima(0)[:2] == [255, 511] and maxima(0)[-1] == 2999 and maxima(1)[0] == 5255 and maxima(2)[0] == 510
    assert hand.ix.lens[0] % 256 == 184 and hand.ix.lens[1] % 256 == 160
    nb = lambda t, r: RR.n_blocks_in_range(hand.blocks, t, *r)  # noqa: E731
    assert nb(0, (300, 400)) == 1 and nb(0, (255, 600)) == 3 and nb(0, (256, 600)) == 2 and nb(0, (100, 256)) == 1
    assert nb(2, (100, 511)) == 1 and nb(2, (100, 512)) == 2 and nb(2, (100, 513)) == 2
    assert nb(1, (4000, 5000)) == 1 and nb(1, (4000, 5001)) == 1  # (a list's first block has base 0: in range up to its max)
    # the positional rule is the record rule, on the index's own records: max >= lo and base < hi
    for lo, hi in HAND_RANGES.values():
        for t in range(5):
            rec = hand.blocks[hand.blocks["list"] == t]
            by_record = int(((rec["max"].astype(np.int64) >= lo) & (rec["base"].astype(np.int64) < hi)).sum()) if lo < hi else 0
            assert by_record == nb(t, (lo, hi)), (t, lo, hi)
    # the gap and after a: a has no block, b has one; before b: both have one (b's first block, of which nothing is in range)
    assert nb(0, (3000, 5000)) == 0 and nb(1, (3000, 5000)) == 1
    assert nb(0, (10, 50)) == 1 and nb(1, (10, 50)) == 1 and nb(0, (6000, 6100)) == 0 and nb(1, (6000, 6100)) == 2
    for r, n_or in (((10, 50), 40), ((6000, 6100), 100), ((3000, 5000), 0)):
        got = hand.run("or", [[0, 1]], [r], 10)
        assert int(got[3][0]) == n_or and got[4] == nb(0, r) + nb(1, r)
        got = hand.run("and", [[0, 1]], [r], 10)
        assert int(got[3][0]) == 0 and int(got[0][0]) == 0 and got[4] == nb(0, r)  # (a is the rarer list)
    # a repeated term weighs twice: every score of [0, 0] above [0]'s, the documents the same
    one, two = hand.run("or", [[0]], [(300, 400)], 10), hand.run("or", [[0, 0]], [(300, 400)], 10)
    assert np.array_equal(one[2], two[2]) and (two[1] > one[1]).all()


@pytest.mark.parametrize("entry", ENTRIES)
def test_unrestricted_is_the_unranged_entry_bit_for_bit(hand, device, small_corpus, entry):
    for r, qs in ((hand, HAND_QUERIES), (None, None)):
        own = r is None
        if own:
            ix = get_index(small_corpus, host.SINGLE_PACKED)
            r = Ranged(device, ix, host.SINGLE_PACKED)
            qs = reference_queries(len(ix.lens))[:150] + heavy_queries(ix.lens, 20) + [[], [0]]
        for k in (10, 1000):
            want = r.unranged(entry, qs, k)
            for ranges in (None, [ALL] * len(qs)):
                got = r.run(entry, qs, ranges, k)
                _assert_equal(got[:3], want)
                assert np.array_equal(np.minimum(got[3], k), want[0])
                assert got[4] == r.want_blocks(entry, qs, None)
                assert r.run(entry, qs, ranges, k, stats=False)[0].tolist() == want[0].tolist()
            if entry == "or":  # every block of the queries' distinct terms
                lens = r.ix.lens.astype(np.int64)
                assert got[4] == sum(int(((lens[sorted(set(q))] + 255) // 256).sum()) for q in qs if len(q))
        if own:
            r.close()


# ---- the batch: every query its own range ---------------------------------------------------------------------------
_EVERY = {}  # {corpus: {(entry, query): every match}}: the model's matches, shared by the three kinds


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_matches():
    yield
    _EVERY.clear()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_is_bit_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Ranged(device, ix, kind, every=_EVERY.setdefault(corpus_name, {}))
    qs, ranges = RR.ranged_batch(reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 60), r.num_docs)
    for entry in ENTRIES:
        for k in (10, 1, 1000):
            got = r.check(entry, qs, ranges, k, corpus_name)
        assert int(got[3].sum()) > 500, "the batch matches something"
        # one-query calls: the same rows and the query's own blocks
        for i in range(0, len(qs), 41):
            one = r.check(entry, [qs[i]], ranges[i:i + 1], 1000, (corpus_name, i))
            assert _same_row(one, got, i)
    r.close()


@pytest.mark.parametrize("s", [2, 7])
def test_slices_merge_to_the_unranged_answer_on_the_device(device, small_corpus, s):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranged(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:100] + heavy_queries(ix.lens, 20) + [[], [0]]
    for entry in ENTRIES:
        for k in (10, 1000):
            want = r.unranged(entry, qs, k)
            # one call: every query under every slice
            cuts = RR.slices(0, r.num_docs, s)
            got = r.run(entry, [q for q in qs for _ in cuts], [c for _ in qs for c in cuts], k)
            for i in range(len(qs)):
                parts = [tuple(a[i * s + j] for a in got[:4]) for j in range(s)]
                n, sc, ids = RR.merge_topk(parts, k)
                assert n == want[0][i] and np.array_equal(sc.view(np.uint32), want[1][i].view(np.uint32)) and np.array_equal(ids, want[2][i])
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    """query_or_pass_pages cuts the OR call into passes sized by the blocks IN RANGE. The passes themselves are not
    observable; blocks_decoded is, and it is what the passes are sized by."""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranged(device, ix, kind)
    qs, ranges = RR.ranged_batch(reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2) + [[], [0]], r.num_docs)
    narrow = np.array([(r.num_docs // 3, r.num_docs // 3 + 1 + r.num_docs // 64)] * len(qs), dtype=np.uint32)
    want = {name: r.want("or", qs, rg, 10) for name, rg in (("own", ranges), ("narrow", narrow), ("all", None))}
    device.set_option("query_or_pass_pages", pass_pages)
    blocks = {}
    for name, rg in (("own", ranges), ("narrow", narrow), ("all", None)):
        got = r.check("or", qs, rg, 10, name)
        blocks[name] = got[4]
        back = r.run("or", qs[::-1], rg[::-1] if rg is not None else None, 10)
        assert all(np.ascontiguousarray(b[::-1]).tobytes() == np.ascontiguousarray(w).tobytes() for b, w in zip(back[:4], want[name]))
        assert back[4] == got[4]
        r.check("and", qs, rg, 10, name)
    assert 0 < blocks["narrow"] < blocks["own"] < blocks["all"]  # (a narrower range: fewer pages, so no more passes)
    r.close()


# ---- docIDs at the top of the u32 range ------------------------------------------------------------------------------
def test_ranges_at_the_top_of_the_docid_space(device):
    kind = host.SINGLE_PACKED
    lists = [np.arange(TOP - 599, TOP + 1, dtype=np.uint64).astype(np.uint32), np.array([0, 5, TOP], dtype=np.uint32),
             np.arange(TOP - 298, TOP + 1, 2, dtype=np.uint64).astype(np.uint32),
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
    for rg in ((0xFFFFFF00, 0xFFFFFFFF), (0xFFFFFFFE, 0xFFFFFFFF), ((1 << 31) - 10, (1 << 31) + 10), (0, 6), ALL, (TOP, TOP)):
        for entry in ENTRIES:
            fn = qi.ranked_or_range_queries if entry == "or" else qi.ranked_and_range_queries
            for k in (10, 1000):
                got = fn(h.fd, wand, qs, [rg] * len(qs), k=k, with_stats=True)
                want = [RR.top_in_range(RR.every_match(bl, q, nl, num_docs, entry == "and"), rg[0], rg[1], k) for q in qs]
                assert got[0].tolist() == [w[0] for w in want] and got[3].tolist() == [w[3] for w in want], (rg, entry)
                assert np.array_equal(got[1].view(np.uint32), np.stack([w[1] for w in want]).view(np.uint32)), (rg, entry)
                assert np.array_equal(got[2], np.stack([w[2] for w in want])), (rg, entry)
            if rg == (0xFFFFFFFE, 0xFFFFFFFF):
                assert got[3].tolist()[:6] == [1] * 6 and got[2][2][0] == TOP  # (every one of the three lists holds it)
    qi.close()
    wand.close()


# ---- errors, and two threads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, entry):
    lib = device._lib
    call = getattr(lib, f"dint_ranked_{entry}_range_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    rg = np.array([[0, 100]], dtype=np.uint32)

    def attempt(k, terms_, counts_null=False):
        counts = np.full(1, 77, dtype=np.uint64)
        matches = np.full(1, 77, dtype=np.uint64)
        scores = np.full(1025, -1.0, dtype=np.float32)
        docids = np.full(1025, 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs.ctypes.data, rg.ctypes.data, 1,
                  None if counts_null else counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                  C.byref(blocks), None)
        untouched = counts[0] == 77 and matches[0] == 77 and (scores == -1.0).all() and (docids == 77).all() and blocks.value == 77
        return st, untouched

    assert attempt(0, terms) == (DINT_ERR_ARG, True)
    assert attempt(1025, terms) == (DINT_ERR_ARG, True)
    assert attempt(10, np.array([0, 5], dtype=np.uint32)) == (DINT_ERR_ARG, True)  # a term >= n_lists
    assert attempt(10, terms, counts_null=True) == (DINT_ERR_ARG, True)
    st, untouched = attempt(10, terms)
    assert st == 0 and not untouched
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            hand.run(entry, [[0]], [(0, 10)], bad_k)
    with pytest.raises(device.DintError):
        hand.run(entry, [[5]], [(0, 10)], 10)
    # nullable outputs: matches, docids and blocks_decoded
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    assert call(hand.qi._h, hand.fd._h, hand.wand._h, 10, terms.ctypes.data, offs.ctypes.data, rg.ctypes.data, 1, counts.ctypes.data,
                None, scores.ctypes.data, None, None, None) == 0
    want = hand.want(entry, [[0, 1]], [(0, 100)], 10)
    assert counts[0] == want[0][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))


def test_two_threads_on_one_handle(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranged(device, ix, kind)
    qs, ranges = RR.ranged_batch(reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8), r.num_docs)
    want = {e: r.want(e, qs, ranges, 10) for e in ENTRIES}
    plain = {e: r.unranged(e, qs, 10) for e in ENTRIES}
    for e in ENTRIES:
        _assert_equal(plain[e], r.want(e, qs, None, 10)[:3])
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine, other = ENTRIES[which], ENTRIES[1 - which]
            for _ in range(3):
                got = r.run(mine, qs, ranges, 10)
                assert all(np.array_equal(g.view(np.uint32), w.view(np.uint32)) for g, w in zip(got[:4], want[mine]))
                _assert_equal(r.unranged(other, qs, 10), plain[other])
        except Exception as e:  # (reported below)
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    r.close()
