"""The wand data's BM25 maxima from the index on the GPU (dint_index_max_weights): max_term_weight equal to
dinth_wand_data's bit for bit and block_max_weight equal to the block model's (tests/blockmax.py) bit for bit, for the three
dictionary kinds, under passes of 1, 2 and 7 pages, and on a hand-made index whose lists have 1 .. 513 postings with each
list's best posting moved through the slots where a reduction can lose it. (An empty list is not among them: the builder
writes one as zero bytes, which the block table reads as the next list's blocks.)"""
import ctypes as C

import numpy as np
import pytest

import blockmax
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_gpu_query_fuzz import HandIndex
from test_gpu_ranked_queries import Ranked
from test_index_cpu import get_index

pytestmark = pytest.mark.gpu

DINT_ERR_ARG = -1
PASSES = [None, 1, 2, 7]


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_maxima(got_mtw, got_bmw, want_mtw, want_bmw, what):
    assert np.array_equal(bits(got_bmw), bits(want_bmw)), (what, np.flatnonzero(bits(got_bmw) != bits(want_bmw))[:8])
    assert np.array_equal(bits(got_mtw), bits(want_mtw)), (what, np.flatnonzero(bits(got_mtw) != bits(want_mtw))[:8])


@pytest.mark.parametrize("pass_pages", PASSES)
@pytest.mark.parametrize("kind", [host.SINGLE_PACKED, host.RECTANGULAR, host.MULTI_PACKED])
def test_equal_to_dinth_wand_data_and_the_block_model(device, small_corpus, kind, pass_pages):
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    _, want_mtw = host.wand_data(r.sizes, ix.docids, ix.freqs, ix.lens)
    want_bmw = blockmax.block_max_weights(ix.docids, ix.freqs, ix.bounds, r.norm_lens)
    assert want_bmw.size == len(r.qi.blocks) > 7
    if pass_pages:
        device.set_option("query_or_pass_pages", pass_pages)
    mtw, bmw = r.qi.max_weights(r.fd, r.wand, with_blocks=True)
    assert_maxima(mtw, bmw, want_mtw, want_bmw, (kind, pass_pages))
    assert np.array_equal(bits(r.qi.max_weights(r.fd, r.wand)), bits(want_mtw))  # block_max_weight null
    r.close()


LENS = (1, 63, 64, 65, 255, 256, 257, 513)
PLACES = ("slot0", "slot63", "slot64", "slot255", "last_block", "pass_start")


def best_position(n: int, place: str) -> int:
    """Where list of n postings gets its best posting: a slot of its first block (its last posting if the list is shorter), the
    last posting (the short last block), or the first slot of its last block — blocks 7 (list of 257) and 10 (list of 513) of
    the table, which begin a pass under 1-page passes, and block 10 under 2-page passes too."""
    if place == "last_block":
        return n - 1
    if place == "pass_start":
        return (n - 1) // 256 * 256
    return min(int(place[4:]), n - 1)


def hand_index(device, kind, place):
    r = np.random.default_rng(5)
    num_docs = 4000
    lists, freqs = [], []
    for n in LENS:
        lists.append(np.sort(r.choice(num_docs, n, replace=False)).astype(np.uint32))
        f = r.integers(1, 4, n).astype(np.uint32)
        f[best_position(n, place)] = 1000
        freqs.append(f)
    sizes = r.integers(1, 200, num_docs).astype(np.uint32)
    sizes[::7] = 0  # a class of documents of length 0: norm_len 0
    nl, mtw = host.wand_data(sizes, np.concatenate(lists), np.concatenate(freqs), np.array(LENS, dtype=np.uint32))
    assert (nl[::7] == 0).all()
    return HandIndex(device, kind, lists, freqs, num_docs, nl), mtw


@pytest.mark.parametrize("place", PLACES)
def test_list_lengths_around_the_block_and_every_place_of_the_best_posting(device, place):
    h, want_mtw = hand_index(device, host.SINGLE_PACKED, place)
    want_bmw = blockmax.block_max_weights(h.docids, h.freqs, h.bounds, h.nl)
    assert want_bmw.size == 11
    # the best posting is the list's maximum, and sits in the block it was put in
    first = blockmax.block_firsts(h.bounds)
    for t, n in enumerate(LENS):
        assert want_bmw[first[t] + best_position(n, place) // 256] == want_mtw[t] > 0.99
    for pass_pages in PASSES:
        if pass_pages:
            device.set_option("query_or_pass_pages", pass_pages)
        mtw, bmw = h.qi.max_weights(h.fd, h.wand, with_blocks=True)
        assert_maxima(mtw, bmw, want_mtw, want_bmw, (place, pass_pages))
    h.close()


def test_twice_on_one_handle_between_other_query_calls(device, small_corpus):
    kind = host.MULTI_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    _, want_mtw = host.wand_data(r.sizes, ix.docids, ix.freqs, ix.lens)
    want_bmw = blockmax.block_max_weights(ix.docids, ix.freqs, ix.bounds, r.norm_lens)
    qs = reference_queries(len(ix.lens))[:60] + heavy_queries(ix.lens, 10)
    and_before = r.qi.and_queries(qs)
    first = r.qi.max_weights(r.fd, r.wand, with_blocks=True)
    assert_maxima(*first, want_mtw, want_bmw, "first")
    # the workspaces are the query calls' own: they answer as before, and so does this call after them
    assert np.array_equal(r.qi.and_queries(qs), and_before)
    or_counts = r.qi.or_queries_with_freqs(r.fd, qs)
    ranked_before = r.qi.ranked_or_queries(r.fd, r.wand, qs, k=10)
    device.set_option("query_or_pass_pages", 3)
    second = r.qi.max_weights(r.fd, r.wand, with_blocks=True)
    assert_maxima(*second, want_mtw, want_bmw, "second")
    device.reset_options()
    again = r.qi.or_queries_with_freqs(r.fd, qs)
    assert np.array_equal(again[0], or_counts[0]) and np.array_equal(again[1], or_counts[1])
    ranked_after = r.qi.ranked_or_queries(r.fd, r.wand, qs, k=10)
    for a, b in zip(ranked_before, ranked_after):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    r.close()


def test_errors(device, small_corpus):
    kind = host.SINGLE_PACKED
    ix = get_index(small_corpus, kind)
    r = Ranked(device, ix, kind)
    lib = device._lib
    mtw = np.zeros(len(ix.lens), dtype=np.float32)
    call = lambda qi, fd, wd, out: lib.dint_index_max_weights(qi, fd, wd, out, None, None)
    assert call(r.qi._h, r.fd._h, r.wand._h, mtw.ctypes.data) == 0
    assert call(r.qi._h, r.fd._h, r.wand._h, None) == DINT_ERR_ARG        # n_lists != 0 and nowhere to write
    assert call(None, r.fd._h, r.wand._h, mtw.ctypes.data) == DINT_ERR_ARG
    assert call(r.qi._h, None, r.wand._h, mtw.ctypes.data) == DINT_ERR_ARG
    assert call(r.qi._h, r.fd._h, None, mtw.ctypes.data) == DINT_ERR_ARG
    other = device.Dictionary(host.MULTI_PACKED, get_index(small_corpus, host.MULTI_PACKED).freqs_dict)
    assert call(r.qi._h, other._h, r.wand._h, mtw.ctypes.data) == DINT_ERR_ARG  # a freqs dictionary of another kind
    short = device.WandData(r.norm_lens[:-1])  # num_docs does not exceed the index's largest docID
    assert call(r.qi._h, r.fd._h, short._h, mtw.ctypes.data) == DINT_ERR_ARG
    with pytest.raises(device.DintError):
        r.qi.max_weights(r.fd, short)
    short.close()
    r.close()
