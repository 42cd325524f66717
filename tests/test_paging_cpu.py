"""Paged ranked queries without a GPU: the entries in the header, the library and the binding, with
DINT_ABI_VERSION still 6; the argument errors that need no device; the model (tests/paging.py) against a document-at-a-time
loop on the keys' bits; and the conditions that tests/test_gpu_paging_fuzz.py demands of its committed seeds, from the model
alone."""
import ctypes as C
import os

import numpy as np
import pytest

import facets as FA
import paging as PG
import ranked
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("dint_ranked_or_paged_queries", "dint_ranked_and_paged_queries")
COLLAPSED = ("dint_ranked_or_collapsed_paged_queries", "dint_ranked_and_collapsed_paged_queries")


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "typedef struct dint_rank_cursor" in header
    for names, n_args in ((PLAIN, 16), (COLLAPSED, 21)):
        for name in names:
            assert f"int {name}(" in header
            assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
            assert hasattr(device.QueryIndex, name[len("dint_"):])
            assert len(getattr(device._lib, name).argtypes) == n_args
    assert hasattr(device.QueryIndex, "ranked_pages")
    assert device._CURSOR.itemsize == 8 and device._CURSOR.fields["docid"][1] == 4  # dint_rank_cursor {float; uint32_t}


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts, skipped, collapsed = (np.full(1, 77, dtype=np.uint64) for _ in range(3))
    scores = np.zeros(2048, dtype=np.float32)
    hits, hit_matches = np.full(2048, 77, dtype=np.uint32), np.full(2048, 77, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    cursor = np.array([(1.0, 3)], dtype=device._CURSOR)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for qi, fd, w, k, cnt in ((None, fake, fake, 10, counts), (fake, None, fake, 10, counts), (fake, fake, None, 10, counts),
                              (fake, fake, fake, 0, counts), (fake, fake, fake, 1025, counts), (fake, fake, fake, 10, None)):
        cnt_p = cnt.ctypes.data if cnt is not None else None
        for after in (None, cursor.ctypes.data):
            for name in PLAIN:
                assert getattr(lib, name)(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, after, 1, cnt_p, None, skipped.ctypes.data,
                                          scores.ctypes.data, None, C.byref(blocks), None) == -1
            for name in COLLAPSED:
                for facets in (None, fake):
                    assert getattr(lib, name)(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, facets, after, 1, cnt_p, None,
                                              collapsed.ctypes.data, skipped.ctypes.data, scores.ctypes.data, None, hits.ctypes.data,
                                              hit_matches.ctypes.data, None, C.byref(blocks), None) == -1
            assert counts[0] == 77 and skipped[0] == 77 and collapsed[0] == 77 and blocks.value == 77 and not scores.any()
            assert (hits == 77).all() and (hit_matches == 77).all()


def test_cursors_are_packed_as_the_struct():
    from dint_amd import device

    assert device._pack_cursors(None, 3) is None
    c = device._pack_cursors([None, (np.float32(1.5), 7), (float("nan"), 0xFFFFFFFF)], 3)
    assert c["score"][0] == np.inf and c["score"][1] == np.float32(1.5) and np.isnan(c["score"][2])
    assert c["docid"].tolist() == [0, 7, 0xFFFFFFFF] and c.tobytes()[8:16] == np.float32(1.5).tobytes() + np.uint32(7).tobytes()


# ---- the model ----------------------------------------------------------------------------------------------------------
def _same(x, y):
    return all(np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes() if isinstance(a, np.ndarray)
               else a == b for a, b in zip(x, y))


def test_the_special_cursors():
    sc = np.array([2.0, 2.0, 1.0, 1.0, 1.0, 0.5], dtype=np.float32)
    ids = np.array([3, 9, 1, 4, 8, 2], dtype=np.uint32)
    m = (sc, ids)
    assert PG.cursor_key(None) == PG.cursor_key((np.inf, 5)) == PG.FROM_START
    for s in (0.0, -0.0, -1.0, -np.inf):
        assert PG.cursor_key((s, 0)) == 0 and PG.page_after(m, None, (s, 0), 4)[::4] == (0, 6)
    assert PG.page_after(m, None, (1e-45, 0), 4)[::4] == (0, 6)  # a subnormal: below every score
    assert PG.page_after(m, None, None, 4)[2].tolist() == [3, 9, 1, 4] and PG.page_after(m, None, (np.inf, 0), 4)[4] == 0
    # a tie across the cursor: a match, a docID that is no match between two matched ones, docID 0 and 0xFFFFFFFF
    assert PG.page_after(m, None, (1.0, 4), 4)[2].tolist() == [8, 2, 0xFFFFFFFF, 0xFFFFFFFF] and PG.page_after(m, None, (1.0, 4), 4)[4] == 4
    assert PG.page_after(m, None, (1.0, 5), 4)[2][:2].tolist() == [8, 2] and PG.page_after(m, None, (1.0, 0), 4)[4] == 2
    assert PG.page_after(m, None, (1.0, 0xFFFFFFFF), 4)[2][0] == 2 and PG.page_after(m, None, (1.0, 0xFFFFFFFF), 4)[4] == 5
    # bits, no tolerance: the next float above a score cuts in front of it, the next below behind it
    up, down = np.nextafter(np.float32(1.0), np.float32(2.0)), np.nextafter(np.float32(1.0), np.float32(0.0))
    assert PG.page_after(m, None, (up, 0xFFFFFFFF), 4)[4] == 2 and PG.page_after(m, None, (down, 0), 4)[4] == 5
    with pytest.raises(AssertionError):
        PG.page_after(m, None, (np.nan, 0), 4)
    for cur in (None, (1.0, 4), (1.0, 5), (up, 7), (down, 0), (0.0, 0), (-0.0, 1), (2.0, 3), (0.5, 2), (np.inf, 1)):
        assert _same(PG.page_after(m, None, cur, 3), PG.page_after_by_loop(m, None, cur, 3)), cur


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_per_document_loop_on_the_bits(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 4, x.size).astype(np.uint32) for x in lists]  # (few distinct freqs: equal scores occur)
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = np.ones(num_docs, dtype=np.float32) if seed % 2 else ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    bl = ranked.BuilderLists(docids, fr, bounds)
    splits = ties = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], []):
            every = PG.CO.every_match(bl, q, nl, num_docs, conjunctive)
            for n_mask in (None, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                sc, ids = PG.in_filter(every, mask)
                cursors = [None, (0.0, 0), (np.inf, 3)] + ([PG.draw_cursor(r, sc, ids, num_docs) for _ in range(8)] if ids.size else [])
                for cur in cursors:
                    for k in (1, 10, 1000):
                        got = PG.page_after(every, mask, cur, k)
                        assert _same(got, PG.page_after_by_loop(every, mask, cur, k)), (q, cur, k)
                        assert got[0] == min(k, got[3] - got[4]) and (np.diff(got[1][:got[0]]) <= 0).all()
                    s, t = PG.split_and_tie(every, mask, cur)
                    splits, ties = splits + s, ties + t
                    g = FA.named_map("clustered", num_docs - 5, 7, seed=seed)
                    got = PG.collapsed_page_after(every, mask, g, 7, cur, 3)
                    assert _same(got, PG.collapsed_page_after_by_loop(every, mask, g, 7, cur, 3)), (q, cur)
                    assert got[0] == min(3, got[4] - got[8]) and got[4] <= got[3]
                # a walk by the last hit: the pages concatenate to the whole order, skipped counts the hits before
                cur, seen = None, []
                while True:
                    n, s, d, m, skipped = PG.page_after(every, mask, cur, 7)
                    assert skipped == len(seen) and m == ids.size
                    seen += d[:n].tolist()
                    if n < 7:
                        break
                    cur = PG.last_hit(n, s, d)
                assert seen == ids.tolist()
    assert splits > 30 and ties > 5


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_seeds_meet_their_conditions():
    """tests/test_gpu_paging_fuzz.py asserts, on the device's own outputs, that the cursor splits the matches in at least half
    of its (case, query) pairs and that in at least one in ten a match with the cursor's score lies on each side of the cut,
    for either plain entry (check_shares there). These are properties of the committed seeds and the draw's weights: replayed
    here from the model, so that they are settled without a device."""
    import test_gpu_paging_fuzz as P

    totals = []
    for seed, kind, ds, fs in P.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = P.Z.F.make_dictionary(r, kind, **ds), P.Z.F.make_dictionary(r, kind, **fs)
        for i in range(P.CASES_PER_DICTIONARY):
            totals.append(P.model_shares(P.Y.draw_collapse_case(Dd, Df, 100 * seed + i)))
    assert len(totals) == 240
    P.check_shares(np.sum(totals, axis=0))
    assert np.sum(totals, axis=0).tolist() == [[4800, 3739, 847], [4800, 2741, 568]]  # (the figures of that file's docstring)
