"""An index checked against its collection on the GPU (dint_check_index; the reference's verify_collection)
against the model of tests/check_index.py: faithful indexes of the three dictionary kinds are clean under passes of 1, 2 and
7 pages; on a hand-made index whose lists have 1 .. 513 postings one mismatch is moved through the slots where a reduction
or a pass boundary can lose it; counts and the first mismatch of many; lengths; a different but valid index; refusals; and
the fuzz generator's indexes under random plants. Every mismatch is planted on the EXPECTED side (a copy of the collection's
arrays handed to the view) or by building a valid index from other postings: no index or dictionary byte is edited."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import check_index as M
import fuzz_streams as F
from dint_amd import host
from test_gpu_query_fuzz import HandIndex
from test_gpu_ranked_queries import Ranked
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
PASSES = [None, 1, 2, 7]
LENS = (1, 63, 64, 65, 255, 256, 257, 513)
NUM_DOCS = 4000
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fuzz_digests.json")))
QUERY = F.query_plan(*GOLDEN["query_plan"])


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


def hand_lists(seed=5):
    r = np.random.default_rng(seed)
    lists = [np.sort(r.choice(NUM_DOCS, n, replace=False)).astype(np.uint32) for n in LENS]
    freqs = [r.integers(1, 40, n).astype(np.uint32) for n in LENS]
    return lists, freqs


@pytest.fixture(scope="module")
def hand(device):
    """The hand index (11 blocks: blocks 6-7 are the list of 257, blocks 8-10 the list of 513), built once and only read."""
    lists, freqs = hand_lists()
    h = HandIndex(device, host.SINGLE_PACKED, lists, freqs, NUM_DOCS, np.ones(NUM_DOCS, dtype=np.float32))
    assert len(h.qi.blocks) == 11
    h.hand_lists, h.hand_freqs = lists, freqs
    yield h
    h.close()


def run(device, qi, fd, view, pass_pages=None, with_freqs=True):
    if pass_pages:
        device.set_option("query_or_pass_pages", pass_pages)
    got = qi.check(fd if with_freqs else None, view.docs, view.freqs if with_freqs else None, view.docs_at,
                   view.freqs_at if with_freqs else None, view.list_len)
    device.reset_options()
    return got


def plant(view, l, i, docid=None, freq=None):
    """One posting of the EXPECTED side changed (the view's arrays are the caller's own copy)."""
    if docid is not None:
        view.docs[int(view.docs_at[l]) + i] = docid
    if freq is not None:
        view.freqs[int(view.freqs_at[l]) + i] = freq


def other(x):
    """A value that differs from x (and from x in more than the low bit)."""
    return (int(x) + 3) & 0xFFFFFFFF


# ---- 1: a faithful index is clean ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pass_pages", PASSES)
@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
def test_a_faithful_index_is_clean(device, small_corpus, kind, pass_pages):
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    assert len(r.qi.blocks) > 7
    b = ix.bounds
    lists = [ix.docids[int(b[i]):int(b[i + 1])] for i in range(len(ix.lens))]
    freqs = [ix.freqs[int(b[i]):int(b[i + 1])] for i in range(len(ix.lens))]
    view = M.view_of(lists, freqs)
    assert run(device, r.qi, r.fd, view, pass_pages) == (0, None)
    assert run(device, r.qi, r.fd, view, pass_pages, with_freqs=False) == (0, None)
    r.close()


# ---- 2: every place a reduction or a pass boundary can lose a mismatch ----------------------------------------------------
# (list, position): slots 0, 63, 64 and 255 of a first and of a middle block; the last posting of a short last block (the
# lists of 1, 65, 255, 257 and 513); the first slot of the list's last block — block 7 (list 6) and block 10 (list 7), which
# begin a pass under 1-page passes, block 10 under 2-page passes too
PLACES = [(7, 0), (7, 63), (7, 64), (7, 255), (7, 256), (7, 256 + 63), (7, 256 + 64), (7, 511), (5, 255), (0, 0), (3, 64), (4, 254),
          (6, 256), (7, 512)]


@pytest.mark.parametrize("what", ["docid", "freq", "both"])
def test_one_mismatch_at_every_place(device, hand, what):
    lists, freqs = hand.hand_lists, hand.hand_freqs
    for n_place, (l, i) in enumerate(PLACES):
        view = M.view_of(lists, freqs)
        # (0xFFFFFFFF is one of the planted docIDs: no docID of an index, a legal word of a view)
        docid = 0xFFFFFFFF if n_place % 3 == 0 else other(lists[l][i])
        plant(view, l, i, docid if what != "freq" else None, other(freqs[l][i]) if what != "docid" else None)
        want = M.check(lists, freqs, view)
        if what == "freq":
            assert want == (1, M.Mismatch(M.FREQ, l, i, other(freqs[l][i]), int(freqs[l][i])))
        else:
            assert want == (1, M.Mismatch(M.DOCID, l, i, docid, int(lists[l][i])))
        for pass_pages in PASSES:
            got = run(device, hand.qi, hand.fd, view, pass_pages)
            assert got[0] == 1 and tuple(got[1]) == tuple(want[1]), (l, i, what, pass_pages, got)
        # docIDs only: the freq alone is not seen
        got = run(device, hand.qi, hand.fd, view, 2, with_freqs=False)
        assert got == ((0, None) if what == "freq" else (1, want[1])), (l, i, what, got)


# ---- 3: count and order ---------------------------------------------------------------------------------------------------
def test_counts_and_the_first_of_many(device, hand):
    lists, freqs = hand.hand_lists, hand.hand_freqs
    total = sum(LENS)
    bounds = np.concatenate([[0], np.cumsum(LENS)])
    r = np.random.default_rng(77)
    views = []
    for K in (1, 2, 64, 300):
        view = M.view_of(lists, freqs)
        for n_plant, g in enumerate(r.choice(total, K, replace=False)):
            l = int(np.searchsorted(bounds, g, side="right")) - 1
            i = int(g - bounds[l])
            mode = n_plant % 3  # docID, freq, both
            plant(view, l, i, other(lists[l][i]) if mode != 1 else None, other(freqs[l][i]) if mode != 0 else None)
        assert M.check(lists, freqs, view)[0] == K
        views.append(view)
    # all 513 postings of the longest list wrong (its three blocks, every wave of them)
    view = M.view_of(lists, freqs)
    at = int(view.docs_at[7])
    view.docs[at:at + 513] += np.uint32(1)
    assert M.check(lists, freqs, view) == (513, M.Mismatch(M.DOCID, 7, 0, int(lists[7][0]) + 1, int(lists[7][0])))
    views.append(view)
    # two mismatches, the lower ordinal in a LATER slot of an earlier block (block 8 slot 200, block 9 slot 5)
    view = M.view_of(lists, freqs)
    plant(view, 7, 256 + 5, docid=other(lists[7][256 + 5]))
    plant(view, 7, 200, freq=other(freqs[7][200]))
    assert M.check(lists, freqs, view) == (2, M.Mismatch(M.FREQ, 7, 200, other(freqs[7][200]), int(freqs[7][200])))
    views.append(view)
    for view in views:
        want = M.check(lists, freqs, view)
        for pass_pages in PASSES:
            got = run(device, hand.qi, hand.fd, view, pass_pages)
            assert got[0] == want[0] and tuple(got[1]) == tuple(want[1]), (pass_pages, got, want)
        want = M.check(lists, freqs, view, with_freqs=False)
        assert run(device, hand.qi, hand.fd, view, 7, with_freqs=False) == want


# ---- 4: lengths -------------------------------------------------------------------------------------------------------------
def test_lengths(device, hand):
    lists, freqs = hand.hand_lists, hand.hand_freqs
    for change in ("longer", "shorter"):
        vl, vf = list(lists), list(freqs)
        if change == "longer":
            vl[3] = np.append(lists[3], np.uint32(NUM_DOCS + 5))
            vf[3] = np.append(freqs[3], np.uint32(1))
        else:
            vl[3], vf[3] = lists[3][:-1], freqs[3][:-1]
        view = M.view_of(vl, vf)
        length = M.Mismatch(M.LENGTH, 3, 0, len(vl[3]), 65)
        for planted in (False, True):
            if planted:  # a wrong docID inside the list of wrong length: not compared
                plant(view, 3, 10, docid=other(lists[3][10]))
            assert M.check(lists, freqs, view) == (1, length)
            for pass_pages in PASSES:
                assert run(device, hand.qi, hand.fd, view, pass_pages) == (1, length), (change, planted, pass_pages)
            assert run(device, hand.qi, hand.fd, view, None, with_freqs=False) == (1, length)
    # a LENGTH in list 5 and a DOCID in list 2: the DOCID is first
    vl, vf = list(lists), list(freqs)
    vl[5], vf[5] = lists[5][:-1], freqs[5][:-1]
    view = M.view_of(vl, vf)
    plant(view, 2, 40, docid=other(lists[2][40]))
    want = (2, M.Mismatch(M.DOCID, 2, 40, other(lists[2][40]), int(lists[2][40])))
    assert M.check(lists, freqs, view) == want
    for pass_pages in PASSES:
        assert run(device, hand.qi, hand.fd, view, pass_pages) == want
    # ... and a posting in list 6, behind the length: the LENGTH is first
    view = M.view_of(vl, vf)
    plant(view, 6, 256, freq=other(freqs[6][256]))
    want = (2, M.Mismatch(M.LENGTH, 5, 0, 255, 256))
    assert M.check(lists, freqs, view) == want
    for pass_pages in PASSES:
        assert run(device, hand.qi, hand.fd, view, pass_pages) == want


# ---- 5: a different but valid index -----------------------------------------------------------------------------------------
def test_a_different_but_valid_index(device, hand):
    lists, freqs = hand_lists()
    # one docID moved into the gap behind it (the list stays strictly increasing), one freq changed
    i = int(np.flatnonzero(np.diff(lists[7].astype(np.int64)) > 1)[300])
    assert i > 256
    lists[7] = lists[7].copy()
    lists[7][i] += 1
    freqs[4] = freqs[4].copy()
    freqs[4][100] += 7
    other_index = HandIndex(device, host.SINGLE_PACKED, lists, freqs, NUM_DOCS, np.ones(NUM_DOCS, dtype=np.float32))
    view = M.view_of(hand.hand_lists, hand.hand_freqs)  # the ORIGINAL arrays
    want = (2, M.Mismatch(M.FREQ, 4, 100, int(hand.hand_freqs[4][100]), int(freqs[4][100])))
    assert M.check(lists, freqs, view) == want
    for pass_pages in PASSES:
        assert run(device, other_index.qi, other_index.fd, view, pass_pages) == want
    want = (1, M.Mismatch(M.DOCID, 7, i, int(hand.hand_lists[7][i]), int(lists[7][i])))
    assert run(device, other_index.qi, other_index.fd, view, 1, with_freqs=False) == want
    other_index.close()
    # the index it was built from is still clean
    assert run(device, hand.qi, hand.fd, view) == (0, None)


# ---- 6: refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(device):
    lists, freqs = hand_lists()
    h = HandIndex(device, host.SINGLE_PACKED, lists, freqs, NUM_DOCS, np.ones(NUM_DOCS, dtype=np.float32))
    view = M.view_of(lists, freqs)
    for _ in range(4):  # (a dictionary takes its four schedule workspaces in turn: after four decodes everything is warm)
        assert run(device, h.qi, h.fd, view) == (0, None)
    p = lambda a: None if a is None else a.ctypes.data

    def status(fd, docs, fr, docs_at, freqs_at, list_len, n_lists):
        v = device.CollectionView(p(docs), p(fr), p(docs_at), p(freqs_at), p(list_len), n_lists)
        n, first = C.c_uint64(), device.IndexMismatch()
        return device._lib.dint_check_index(h.qi._h, fd._h if fd is not None else None, C.byref(v), C.byref(n), C.byref(first), None)

    before = device.alloc_count()
    n = len(LENS)
    assert status(h.fd, view.docs, view.freqs, view.docs_at, view.freqs_at, view.list_len, n) == 0
    assert status(h.fd, view.docs, view.freqs, view.docs_at, view.freqs_at, view.list_len, n - 1) == DINT_ERR_ARG
    assert status(h.fd, view.docs, view.freqs, view.docs_at, view.freqs_at, view.list_len, n + 1) == DINT_ERR_ARG
    assert status(None, view.docs, view.freqs, view.docs_at, view.freqs_at, view.list_len, n) == DINT_ERR_ARG  # freqs, no dictionary
    assert status(h.fd, view.docs, None, view.docs_at, None, view.list_len, n) == DINT_ERR_ARG                 # a dictionary, no freqs
    assert status(h.fd, None, view.freqs, view.docs_at, view.freqs_at, view.list_len, n) == DINT_ERR_ARG       # null arrays
    assert status(h.fd, view.docs, view.freqs, None, view.freqs_at, view.list_len, n) == DINT_ERR_ARG
    assert status(h.fd, view.docs, view.freqs, view.docs_at, None, view.list_len, n) == DINT_ERR_ARG
    assert status(h.fd, view.docs, view.freqs, view.docs_at, view.freqs_at, None, n) == DINT_ERR_ARG
    # every refusal came before anything was launched or allocated, and a warm check allocates nothing either
    assert device.alloc_count() == before
    multi = device.Dictionary(host.MULTI_PACKED, host.build_dictionary(host.MULTI_PACKED, host.Collection(
        np.concatenate(freqs) - np.uint32(1), np.array(LENS, dtype=np.uint32))))
    before = device.alloc_count()
    assert status(multi, view.docs, view.freqs, view.docs_at, view.freqs_at, view.list_len, n) == DINT_ERR_ARG  # another kind
    with pytest.raises(device.DintError):
        h.qi.check(multi, view.docs, view.freqs, view.docs_at, view.freqs_at, view.list_len)
    assert device.alloc_count() == before
    # the handle still answers: a clean check, a mismatch, and a query call
    assert run(device, h.qi, h.fd, view, 2) == (0, None)
    plant(view, 6, 256, docid=0xFFFFFFFF)
    assert run(device, h.qi, h.fd, view, 2) == (1, M.Mismatch(M.DOCID, 6, 256, 0xFFFFFFFF, int(lists[6][256])))
    assert device.alloc_count() == before
    assert int(h.qi.and_queries([[6, 7]])[0]) == np.intersect1d(lists[6], lists[7]).size
    before = device.alloc_count()
    multi.close()
    h.close()
    assert device.alloc_count() == before  # (closing allocates nothing; the handle's staging buffers go with it)


# ---- 7: the fuzz generator's indexes under random plants -------------------------------------------------------------------------
@pytest.mark.parametrize("case", QUERY, ids=lambda c: f"seed{c[0]}")
def test_fuzz_case(device, case):
    Dd, Df, X = F.build_query_case(case)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    qi = device.QueryIndex(dd, X.index, X.offsets)
    b = X.bounds
    n_lists = len(b) - 1
    lists = [X.docids[int(b[i]):int(b[i + 1])] for i in range(n_lists)]
    freqs = [X.freqs[int(b[i]):int(b[i + 1])] for i in range(n_lists)]
    r = np.random.default_rng(case[0] + 1)
    for rnd in range(3):
        view = M.view_of(lists, freqs)
        for g in r.choice(int(b[-1]), int(r.choice([0, 1, 3, 40, 2000])), replace=False):
            l = int(np.searchsorted(b, g, side="right")) - 1
            i = int(g - b[l])
            mode = int(r.integers(3))
            plant(view, l, i, other(lists[l][i]) if mode != 1 else None, other(freqs[l][i]) if mode != 0 else None)
        vl = view.list_len
        for l in r.choice(n_lists, int(r.choice([0, 0, 1, 2])), replace=False):  # a list of wrong length (its postings stay where they are)
            vl[l] -= 1
        pass_pages = [None, 1, 2, 7, 50][int(r.integers(5))]
        with_freqs = bool(r.integers(4))
        want = M.check(lists, freqs, view, with_freqs=with_freqs)
        got = run(device, qi, fd, view, pass_pages, with_freqs=with_freqs)
        assert got == want, (case[0], rnd, pass_pages, with_freqs)
    qi.close()
