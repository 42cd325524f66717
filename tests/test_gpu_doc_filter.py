"""Document-filter ranked queries on the GPU through the C ABI (dint_doc_filter_create, dint_ranked_or_filtered_queries,
dint_ranked_and_filtered_queries): the handle's n_set and live_blocks exact; counts, BM25 scores, docIDs
and match counts bit-equal to the model (tests/doc_filter.py: the unfiltered models filtered by the mask); blocks_decoded
equal to the live blocks of the host block table; a null and an all-ones filter equal to the unfiltered entries, an interval
filter equal to the range entries."""
import ctypes as C
import threading

import numpy as np
import pytest

import doc_filter as DF
import ranked
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_query_high_docids import TOP, HighIndex
from test_gpu_ranked_queries import _assert_equal, _hand_made
from test_gpu_ranked_range import HAND_QUERIES, HAND_RANGES, Ranged
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
KINDS = [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED]
ENTRIES = ("or", "and")
HAND_DOCS = 9000


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


def _bit_equal(got, want, what=None):
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


class Filtered(Ranged):
    """Ranged (an index, its freqs dictionary and wand data on the device, the range entries and the model's matches) with
    the two filtered entries, their model and the live blocks of the host block table."""

    def filter(self, mask, num_docs=None):
        return self.qi.doc_filter(mask, num_docs)

    def run_f(self, entry, qs, f, k, stats=True):
        fn = self.qi.ranked_or_filtered_queries if entry == "or" else self.qi.ranked_and_filtered_queries
        return fn(self.fd, self.wand, qs, f, k=k, with_stats=stats)

    def want_f(self, entry, qs, mask, k):
        out = [DF.top_in_filter(self.matches_of(entry, q), mask, k) for q in qs]
        return (np.array([o[0] for o in out], dtype=np.uint64), np.stack([o[1] for o in out]) if out else np.zeros((0, k), np.float32),
                np.stack([o[2] for o in out]) if out else np.zeros((0, k), np.uint32), np.array([o[3] for o in out], dtype=np.uint64))

    def per_list(self, mask):
        """per list, its live blocks under the mask (None: every block) — what want_blocks_f sums"""
        return DF.live_per_list(self.blocks, DF.live_blocks(self.blocks, mask) if mask is not None else None, len(self.ix.lens))

    def want_blocks_f(self, entry, qs, mask, per_list=None):
        per_list = per_list if per_list is not None else self.per_list(mask)
        return sum(DF.planned_of(per_list, self.ix.lens, q, entry == "and") for q in qs)

    def check_f(self, entry, qs, mask, k, what=None, f=None, per_list=None):
        """the call under `mask` (through the handle f, or one made and closed here) against the model; per_list: the
        mask's, where the caller has it"""
        own = f is None
        if own:
            f = self.filter(mask)
        got = self.run_f(entry, qs, f, k)
        _bit_equal(got[:4], self.want_f(entry, qs, mask, k), (entry, k, what))
        assert np.array_equal(got[0], np.minimum(got[3], k))
        assert got[4] == self.want_blocks_f(entry, qs, mask, per_list), (entry, k, what)
        if own:
            f.close()
        return got


@pytest.fixture(scope="module")
def hand(device):
    """test_gpu_ranked_range.py's hand-made index: a = 0 .. 2999 (blocks [256 j, 256 j + 255], the last one 2816 .. 2999),
    b = 5000 .. 8999 (its first block has base 0 and max 5255, the last one is 8840 .. 8999), c = the evens (blocks
    [512 j - 1, 512 j + 510]), d = every doc, e = {10, 20, 30, 40}"""
    kind = host.MULTI_PACKED
    r = Filtered(device, _hand_made(device, kind), kind, num_docs=HAND_DOCS, norm_lens=np.ones(HAND_DOCS, dtype=np.float32))
    yield r
    r.close()


# ---- the handle -------------------------------------------------------------------------------------------------------
# 16384 docIDs are one workgroup of the rank directory's scan (256 words), 256 workgroups one round of its grid level
@pytest.mark.parametrize("num_docs", [1, 63, 64, 65, 127, 128, 129, 8999, 9000, 9001, 16384, 16385, 3 * 16384 + 77, 257 * 16384 + 5])
def test_info_is_exact(hand, num_docs):
    r = np.random.default_rng(num_docs)
    for density in (0.5, 1.0 / 64, 1.0, 0.0):
        mask = r.random(num_docs) < density
        f = hand.filter(mask)
        info = f.info
        live = DF.live_blocks(hand.blocks, mask)
        assert (info.num_docs, info.n_set, info.n_blocks, info.live_blocks) == (num_docs, int(mask.sum()), len(hand.blocks), int(live.sum()))
        f.close()
    # a clustered filter: dead blocks between live ones; and through the words and the docID forms, the same handle
    mask = np.zeros(num_docs, dtype=bool)
    mask[num_docs // 3:num_docs // 3 + 50] = True
    mask[num_docs - 1] = True
    want = (num_docs, int(mask.sum()), len(hand.blocks), int(DF.live_blocks(hand.blocks, mask).sum()))
    words = np.packbits(np.concatenate([mask, np.zeros(-num_docs % 64, dtype=bool)]), bitorder="little").view("<u8")
    for form, n in ((mask, None), (words, num_docs), (np.flatnonzero(mask), num_docs)):
        f = hand.filter(form, n)
        info = f.info
        assert (info.num_docs, info.n_set, info.n_blocks, info.live_blocks) == want
        f.close()


def test_bits_past_num_docs_are_ignored(hand):
    for num_docs in (1, 65, 3001, 8990):
        words = np.full(-(-num_docs // 64), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # (the last word: garbage past num_docs)
        f = hand.filter(words, num_docs)
        mask = np.ones(num_docs, dtype=bool)
        assert f.info.n_set == num_docs and f.info.live_blocks == int(DF.live_blocks(hand.blocks, mask).sum())
        for entry in ENTRIES:
            hand.check_f(entry, HAND_QUERIES, mask, 1000, num_docs, f=f)  # (documents num_docs .. 64 * words - 1 are not matches)
        f.close()


def test_num_docs_below_above_and_zero(hand):
    r = np.random.default_rng(4)
    for num_docs in (5100, HAND_DOCS + 5000):  # below (inside b's first block) and above the largest docID
        mask = r.random(num_docs) < 0.3
        for entry in ENTRIES:
            hand.check_f(entry, HAND_QUERIES, mask, 10, num_docs)
    for form in (np.zeros(0, dtype=bool), np.zeros(0, dtype=np.uint64), []):
        f = hand.filter(form)
        info = f.info
        assert (info.num_docs, info.n_set, info.live_blocks) == (0, 0, 0)
        for entry in ENTRIES:  # an empty filter selects nothing and decodes nothing
            got = hand.run_f(entry, HAND_QUERIES, f, 10)
            assert not got[0].any() and not got[3].any() and not got[1].any() and (got[2] == 0xFFFFFFFF).all() and got[4] == 0
        f.close()
    mask = np.zeros(HAND_DOCS, dtype=bool)  # bits, none set
    for entry in ENTRIES:
        assert hand.check_f(entry, HAND_QUERIES, mask, 10)[4] == 0


def test_only_63_64_65(hand):
    mask = DF.as_mask([63, 64, 65], HAND_DOCS)
    f = hand.filter([63, 64, 65], HAND_DOCS)
    assert f.info.n_set == 3
    for entry in ENTRIES:
        got = hand.check_f(entry, HAND_QUERIES, mask, 10, f=f)
        assert got[3].tolist()[:3] == ([3, 3, 3] if entry == "or" else [0, 0, 3])  # [0, 1], [1, 0], [3]
        assert got[2][2][:3].tolist() == [63, 64, 65]
    f.close()


# ---- the live rule ----------------------------------------------------------------------------------------------------
HAND_FILTERS = {
    "a block's max": [255],
    "a block's base": [256],
    "c's second block's base, which c does not hold": [511],
    "a gap that holds no posting": [4000],           # (b's first block, base 0: live, decoded, matches nothing)
    "just past a's last docID": [3000],
    "a's short last block": [2999],
    "b's and d's short last block": [8999],
    "the list of one block": [20],
    "past e's only block": [41],
    "a dead block between two live ones": [100, 700],
    "dead blocks between live ones, all lists": [3, 700, 2900, 5300, 7000, 8998],
    "a has no live block, b and d have": [6000],
    "a few in every block of a": list(range(5, 3000, 128)),
}


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("name", list(HAND_FILTERS))
def test_live_rule(hand, entry, name):
    mask = DF.as_mask(HAND_FILTERS[name], HAND_DOCS)
    f = hand.filter(mask)
    assert f.info.live_blocks == int(DF.live_blocks(hand.blocks, mask).sum())
    for k in (10, 1000):
        got = hand.check_f(entry, HAND_QUERIES, mask, k, name, f=f)
    for i in (0, 4, 8, 11):  # one query per call: the same rows
        one = hand.check_f(entry, [HAND_QUERIES[i]], mask, 1000, (name, i), f=f)
        assert _same_row(one, got, i)
    f.close()


def test_live_cases_are_what_they_are_said_to_be(hand):
    rec = lambda t: hand.blocks[hand.blocks["list"] == t]  # noqa: E731
    live = lambda t, name: DF.live_blocks(rec(t), DF.as_mask(HAND_FILTERS[name], HAND_DOCS)).tolist()  # noqa: E731
    assert rec(0)["max"][:3].tolist() == [255, 511, 767] and rec(0)["base"][:3].tolist() == [0, 256, 512]
    assert rec(1)["base"][0] == 0 and rec(1)["max"][0] == 5255 and rec(2)["base"][1] == 511 and rec(4)["max"].tolist() == [40]
    assert live(0, "a block's max")[:2] == [True, False] and live(0, "a block's base")[:3] == [False, True, False]
    assert live(2, "c's second block's base, which c does not hold")[:3] == [False, True, False]
    assert not any(live(0, "a gap that holds no posting")) and live(1, "a gap that holds no posting") == [True] + [False] * 15
    assert not any(live(0, "just past a's last docID")) and live(0, "a's short last block") == [False] * 11 + [True]
    assert live(4, "the list of one block") == [True] and live(4, "past e's only block") == [False]
    assert live(0, "a dead block between two live ones")[:4] == [True, False, True, False]
    assert not any(live(0, "a has no live block, b and d have")) and any(live(1, "a has no live block, b and d have"))
    # the gap: b's first block is decoded and matches nothing; a, with no live block, keeps its place in [0, 1] and [0, 3]
    f = hand.filter(HAND_FILTERS["a gap that holds no posting"], HAND_DOCS)
    got = hand.run_f("or", [[1], [0, 1], [0, 3]], f, 10)
    assert got[3].tolist() == [0, 0, 1] and got[4] == 1 + 1 + 1 and got[2][2][0] == 4000
    f.close()
    # the dead block between two live ones, as the scored list (a's own slots) and as a probed list (d's slots probe a)
    f = hand.filter(HAND_FILTERS["a dead block between two live ones"], HAND_DOCS)
    got = hand.run_f("or", [[0], [0, 3], [3, 0, 2]], f, 10)
    assert got[3].tolist() == [2, 2, 2] and got[2][1][:2].tolist() == [100, 700] and got[4] == 2 + (2 + 2) + (2 + 2 + 2)
    both = hand.run_f("or", [[0, 3]], f, 10)[1][0][:2]
    assert (both > hand.run_f("or", [[0]], f, 10)[1][0][:2]).all()  # (700 was found in a's second PAGE, its third block)
    f.close()


# ---- the equivalences, bit for bit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_null_and_all_ones_are_the_unfiltered_entry(hand, device, small_corpus, entry):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    own = Filtered(device, ix, host.SINGLE_PACKED)
    for r, qs in ((hand, HAND_QUERIES), (own, reference_queries(len(ix.lens))[:150] + heavy_queries(ix.lens, 20) + [[], [0]])):
        top = int(r.ix.docids.max()) + 1
        for k in (10, 1000):
            want = r.unranged(entry, qs, k)
            for num_docs in (None, top, top + 1, top + 777):  # no filter; every bit up to exactly / past the largest docID + 1
                f = r.filter(np.ones(num_docs, dtype=bool)) if num_docs else None
                got = r.run_f(entry, qs, f, k)
                _assert_equal(got[:3], want)
                assert np.array_equal(np.minimum(got[3], k), want[0])
                assert got[4] == r.want_blocks_f(entry, qs, None)
                _bit_equal(r.run_f(entry, qs, f, k, stats=False), want)
                if f is not None:
                    assert f.info.live_blocks == f.info.n_blocks == len(r.blocks)
                    f.close()
    own.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_interval_filter_is_the_range_entry(hand, entry):
    for name, (lo, hi) in HAND_RANGES.items():
        lo_, hi_ = min(lo, HAND_DOCS + 100), min(hi, HAND_DOCS + 100)
        mask = np.zeros(HAND_DOCS + 100, dtype=bool)
        mask[lo_:hi_] = True
        f = hand.filter(mask)
        for k in (10, 1000):
            got = hand.run_f(entry, HAND_QUERIES, f, k)
            want = hand.run(entry, HAND_QUERIES, [(lo, hi)] * len(HAND_QUERIES), k)
            _bit_equal(got[:4], want[:4], name)
            assert got[4] == want[4], name
        f.close()


# ---- the batch --------------------------------------------------------------------------------------------------------
_EVERY = {}  # {corpus: {(entry, query): every match}}: the model's matches, shared by the three kinds


@pytest.fixture(scope="module", autouse=True)
def _drop_the_shared_matches():
    yield
    _EVERY.clear()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("corpus_name", ["small_corpus", "dense_corpus", "sparse_corpus"])
def test_batch_is_bit_equal_to_the_model(device, request, kind, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), kind)
    r = Filtered(device, ix, kind, every=_EVERY.setdefault(corpus_name, {}))
    qs = reference_queries(len(ix.lens))[::2] + heavy_queries(ix.lens, 30)
    term = int(np.argmax(ix.lens))
    of_term = ix.docids[int(ix.bounds[term]):int(ix.bounds[term + 1])]
    unfiltered = {e: r.want_blocks_f(e, qs, None) for e in ENTRIES}
    matched = {e: 0 for e in ENTRIES}
    for name in DF.BATCH_FILTERS:
        mask = DF.batch_filter(name, DF.batch_num_docs(r.num_docs), ix.docids, of_term)
        f = r.filter(mask)
        per_list = r.per_list(mask)
        assert f.info.n_set == int(mask.sum()) and f.info.live_blocks == int(per_list.sum())
        for entry in ENTRIES:
            for k in ((10, 1, 1000) if name == "half" else (1000,)):
                got = r.check_f(entry, qs, mask, k, (corpus_name, name), f=f, per_list=per_list)
            assert got[4] <= unfiltered[entry] and int(got[3].sum()) > 0
            matched[entry] += int(got[3].sum())
            if name == "runs":
                assert got[4] < unfiltered[entry]  # (clustered: whole blocks are skipped)
            for i in range(0, len(qs), 67):  # one-query calls: the same rows and the query's own blocks
                one = r.check_f(entry, [qs[i]], mask, 1000, (corpus_name, name, i), f=f, per_list=per_list)
                assert _same_row(one, got, i)
        f.close()
    assert matched["or"] > 5000 and matched["and"] > 500, "the batch matches something"  # (tests/test_doc_filter_cpu.py)
    r.close()


@pytest.mark.parametrize("pass_pages", [1, 2, 7])
def test_a_call_in_many_passes(device, small_corpus, pass_pages):
    """query_or_pass_pages cuts the OR call into passes sized by the LIVE blocks. The passes themselves are not observable;
    blocks_decoded is, and it is what the passes are sized by."""
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Filtered(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:120] + heavy_queries(ix.lens, 30, seed=2) + [[], [0]]
    assert len(r.blocks) > 512  # (the live rank's scan spans workgroups)
    masks = {name: DF.batch_filter(name, r.num_docs, ix.docids, None) for name in ("half", "runs")}
    want = {name: r.want_f("or", qs, m, 10) for name, m in masks.items()}
    device.set_option("query_or_pass_pages", pass_pages)
    blocks = {}
    for name, m in masks.items():
        f = r.filter(m)
        got = r.check_f("or", qs, m, 10, name, f=f)
        blocks[name] = got[4]
        back = r.run_f("or", qs[::-1], f, 10)
        assert all(np.ascontiguousarray(b[::-1]).tobytes() == np.ascontiguousarray(w).tobytes() for b, w in zip(back[:4], want[name]))
        assert back[4] == got[4]
        r.check_f("and", qs, m, 10, name, f=f)
        f.close()
    assert 0 < blocks["runs"] < blocks["half"]
    r.close()


@pytest.mark.parametrize("entry", ENTRIES)
def test_k_of_one_and_the_largest(hand, entry):
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    for k in (1, 1024):
        got = hand.check_f(entry, HAND_QUERIES, mask, k, f=f)
    assert int(got[0].max()) == 1024 and int(got[3].max()) > 1024
    f.close()


# ---- docIDs at the top of the u32 range -------------------------------------------------------------------------------
def test_docids_near_2_to_the_32(device):
    """An index with docIDs up to 0xFFFFFFFE under a filter whose num_docs is small: every high document is outside the
    bitmap, which is never read past its end (the bound is compared first)."""
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
    lens = np.array([x.size for x in lists])
    qs = [[0], [1], [0, 1], [0, 2], [1, 2], [0, 1, 2], [2, 2, 1], [3], [0, 3], [1, 3], []]
    for members, n in (([0, 5, 6, 99], 100), ([5], 6), ([3, 150], 1000), ([], 0)):
        mask = DF.as_mask(members, n)
        f = qi.doc_filter(mask)
        live = DF.live_blocks(qi.blocks, mask)
        assert f.info.n_set == len(members) and f.info.live_blocks == int(live.sum())
        for entry in ENTRIES:
            fn = qi.ranked_or_filtered_queries if entry == "or" else qi.ranked_and_filtered_queries
            got = fn(h.fd, wand, qs, f, k=10, with_stats=True)
            want = [DF.top_in_filter(DF.every_match(bl, q, nl, num_docs, entry == "and"), mask, 10) for q in qs]
            assert got[0].tolist() == [w[0] for w in want] and got[3].tolist() == [w[3] for w in want], (members, entry)
            assert np.array_equal(got[1].view(np.uint32), np.stack([w[1] for w in want]).view(np.uint32)), (members, entry)
            assert np.array_equal(got[2], np.stack([w[2] for w in want])), (members, entry)
            assert got[4] == sum(DF.planned_blocks(qi.blocks, live, lens, q, entry == "and") for q in qs)
            assert (got[2][got[2] != 0xFFFFFFFF] < n).all()
        f.close()
    qi.close()
    wand.close()


# ---- errors, and two threads ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
def test_errors_write_nothing(device, hand, entry):
    lib = device._lib
    call = getattr(lib, f"dint_ranked_{entry}_filtered_queries")
    terms = np.array([0, 1], dtype=np.uint32)
    offs = np.array([0, 2], dtype=np.uint64)
    mask = DF.batch_filter("half", HAND_DOCS, None, None)
    f = hand.filter(mask)
    other = device.QueryIndex(device.Dictionary(host.MULTI_PACKED, hand.ix.docs_dict), hand.ix.bytes, hand.ix.offsets)
    f_other = other.doc_filter(mask)

    def attempt(k, terms_, filt, counts_null=False):
        counts = np.full(1, 77, dtype=np.uint64)
        matches = np.full(1, 77, dtype=np.uint64)
        scores = np.full(1025, -1.0, dtype=np.float32)
        docids = np.full(1025, 77, dtype=np.uint32)
        blocks = C.c_uint64(77)
        st = call(hand.qi._h, hand.fd._h, hand.wand._h, k, terms_.ctypes.data, offs.ctypes.data, filt._h, 1,
                  None if counts_null else counts.ctypes.data, matches.ctypes.data, scores.ctypes.data, docids.ctypes.data,
                  C.byref(blocks), None)
        untouched = counts[0] == 77 and matches[0] == 77 and (scores == -1.0).all() and (docids == 77).all() and blocks.value == 77
        return st, untouched

    assert attempt(0, terms, f) == (DINT_ERR_ARG, True)
    assert attempt(1025, terms, f) == (DINT_ERR_ARG, True)
    assert attempt(10, np.array([0, 5], dtype=np.uint32), f) == (DINT_ERR_ARG, True)  # a term >= n_lists
    assert attempt(10, terms, f, counts_null=True) == (DINT_ERR_ARG, True)
    assert attempt(10, terms, f_other) == (DINT_ERR_ARG, True)  # a filter of another query index
    st, untouched = attempt(10, terms, f)
    assert st == 0 and not untouched
    for bad_k in (0, 1025):
        with pytest.raises(device.DintError):
            hand.run_f(entry, [[0]], f, bad_k)
    with pytest.raises(device.DintError):
        hand.run_f(entry, [[5]], f, 10)
    with pytest.raises(device.DintError):
        hand.run_f(entry, [[0]], f_other, 10)
    # the handle's own errors: num_docs past 2^32 - 1, a null index, null bits with documents
    h = C.c_void_p(77)
    word = np.zeros(1, dtype=np.uint64)
    assert lib.dint_doc_filter_create(hand.qi._h, word.ctypes.data, 0x100000000, C.byref(h)) == DINT_ERR_ARG
    assert lib.dint_doc_filter_create(None, word.ctypes.data, 10, C.byref(h)) == DINT_ERR_ARG
    assert lib.dint_doc_filter_create(hand.qi._h, None, 10, C.byref(h)) == DINT_ERR_ARG
    assert lib.dint_doc_filter_info_get(None, C.byref(device.DocFilterInfo())) == DINT_ERR_ARG
    # nullable outputs: matches, docids and blocks_decoded
    counts = np.zeros(1, dtype=np.uint64)
    scores = np.zeros(10, dtype=np.float32)
    assert call(hand.qi._h, hand.fd._h, hand.wand._h, 10, terms.ctypes.data, offs.ctypes.data, f._h, 1, counts.ctypes.data,
                None, scores.ctypes.data, None, None, None) == 0
    want = hand.want_f(entry, [[0, 1]], mask, 10)
    assert counts[0] == want[0][0] and np.array_equal(scores.view(np.uint32), want[1][0].view(np.uint32))
    f_other.close()
    other.close()
    f.close()


def test_two_threads_one_handle_one_filter(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Filtered(device, ix, kind)
    qs = reference_queries(len(ix.lens))[:80] + heavy_queries(ix.lens, 8)
    mask = DF.batch_filter("runs", r.num_docs, ix.docids, None) | DF.batch_filter("one in 64", r.num_docs, None, None)
    f = r.filter(mask)
    want = {e: r.want_f(e, qs, mask, 10) for e in ENTRIES}
    plain = {e: r.unranged(e, qs, 10) for e in ENTRIES}
    errors = []

    def worker(which):
        try:
            import torch

            torch.cuda.set_device(0)
            mine, other = ENTRIES[which], ENTRIES[1 - which]
            for _ in range(3):
                got = r.run_f(mine, qs, f, 10)
                _bit_equal(got[:4], want[mine])
                _assert_equal(r.unranged(other, qs, 10), plain[other])
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
