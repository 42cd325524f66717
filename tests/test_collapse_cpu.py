"""Collapsed ranked queries without a GPU: the entries in the header, the library and the binding,
with DINT_ABI_VERSION still 6; the argument errors that need no device; the model (tests/collapse.py) against a
document-at-a-time loop; and the conditions that tests/test_gpu_collapse_fuzz.py demands of its committed seeds, from the
model alone."""
import os

import numpy as np
import pytest

import collapse as CO
import facets as FA
import ranked
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dint_ranked_or_collapsed_queries", "dint_ranked_and_collapsed_queries")


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "8 BYTES PER (QUERY, GROUP)" in " ".join(header.replace("*", " ").split())  # (the per-call table's device memory is stated)
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert hasattr(device.QueryIndex, name[len("dint_"):])
        assert len(getattr(device._lib, name).argtypes) == 19


def test_argument_errors_need_no_device():
    import ctypes as C

    from dint_amd import device

    lib = device._lib
    counts = np.full(1, 77, dtype=np.uint64)
    collapsed = np.full(1, 77, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    hits = np.full(2048, 77, dtype=np.uint32)
    hit_matches = np.full(2048, 77, dtype=np.uint32)
    rows = np.full(8, 77, dtype=np.uint32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for name in ENTRIES:
        call = getattr(lib, name)
        for qi, fd, w, k, cnt in ((None, fake, fake, 10, counts), (fake, None, fake, 10, counts), (fake, fake, None, 10, counts),
                                  (fake, fake, fake, 0, counts), (fake, fake, fake, 1025, counts), (fake, fake, fake, 10, None)):
            for facets in (None, fake):
                for with_rows in (False, True):
                    assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, facets, 1, cnt.ctypes.data if cnt is not None else None,
                                None, collapsed.ctypes.data, scores.ctypes.data, None, hits.ctypes.data, hit_matches.ctypes.data,
                                rows.ctypes.data if with_rows else None, C.byref(blocks), None) == -1
                    assert counts[0] == 77 and collapsed[0] == 77 and blocks.value == 77 and not scores.any()  # nothing is written
                    assert (hits == 77).all() and (hit_matches == 77).all() and (rows == 77).all()


# ---- the model ----------------------------------------------------------------------------------------------------------
def _same(x, y):
    return all(np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes() if isinstance(a, np.ndarray)
               else a == b for a, b in zip(x, y))


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_per_document_loop(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 4, x.size).astype(np.uint32) for x in lists]  # (few distinct freqs: equal scores occur)
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = np.ones(num_docs, dtype=np.float32) if seed % 2 else ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    bl = ranked.BuilderLists(docids, fr, bounds)
    removed = ties = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], [2, 0], []):
            every = CO.every_match(bl, q, nl, num_docs, conjunctive)
            ties += int(every[0].size - np.unique(every[0]).size)
            for n_mask in (None, num_docs, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                for name in FA.MAPS:
                    for n_map, n_groups in ((num_docs, 3), (num_docs // 2, 17), (num_docs + 9, 300)):  # the map: at, below, above
                        g = FA.named_map(name, n_map, n_groups, seed=seed)
                        for k in (1, 10, 1000):
                            got = CO.collapse(every, mask, g, n_groups, k)
                            assert _same(got, CO.collapse_by_loop(every, mask, g, n_groups, k)), (q, name, n_map, k)
                            count, scores, ids, matches, collapsed, hit_groups, hit_matches, row = got
                            assert count == min(collapsed, k) and collapsed <= matches == FA.matches_in(every, mask).size
                            assert np.array_equal(row, FA.row_of(g, n_groups, FA.matches_in(every, mask))[0])
                            # what is kept: a document per group that has a match, and every match in no group
                            assert collapsed == np.count_nonzero(row) + matches - int(row.sum())
                            shown = hit_groups[:count]
                            grouped = shown[shown != CO.DEVICE_NONE]
                            assert np.unique(grouped).size == grouped.size  # at most one hit a group
                            assert (hit_matches[:count][shown == CO.DEVICE_NONE] == 1).all() and not hit_matches[count:].any()
                            assert np.array_equal(hit_matches[:count][shown != CO.DEVICE_NONE], row[grouped])
                            assert (np.diff(scores[:count]) <= 0).all()
                            removed += matches - collapsed
    assert removed > 1000 and ties > 0
    # "none": nothing is removed; "one group": one document is kept, the best of all
    every = CO.every_match(bl, [0, 1], nl, num_docs, False)
    got = CO.collapse(every, None, FA.named_map("none", num_docs, 4), 4, 5)
    assert got[4] == got[3] and np.array_equal(got[2][:got[0]], every[1][np.lexsort((every[1], -every[0]))][:5])
    got = CO.collapse(every, None, FA.named_map("one group", num_docs, 4), 4, 5)
    assert got[:1] + got[3:5] == (1, every[1].size, 1) and got[2][0] == every[1][np.lexsort((every[1], -every[0]))][0] and got[6][0] == every[1].size


def test_equal_scores_go_to_the_smaller_docid():
    sc = np.array([1.0, 2.0, 2.0, 2.0, 0.5, 2.0], dtype=np.float32)
    ids = np.array([7, 9, 3, 5, 1, 4], dtype=np.uint32)
    g = np.array([0, 0, 0, 1, 1, 1, 1, 1, 0, 1], dtype=np.int64)  # 3, 4, 5, 7, 9 -> 1, 1, 1, 1, 1; 1 -> 0
    got = CO.collapse((sc, ids), None, g, 2, 4)
    assert got[0] == 2 and got[2].tolist() == [3, 1, 0xFFFFFFFF, 0xFFFFFFFF] and got[1].tolist() == [2.0, 0.5, 0.0, 0.0]
    assert got[3:5] == (6, 2) and got[5].tolist() == [1, 0, CO.DEVICE_NONE, CO.DEVICE_NONE] and got[6].tolist() == [5, 1, 0, 0]
    assert got[7].tolist() == [1, 5]
    short = CO.collapse((sc, ids), None, g[:5], 2, 4)  # the map ends at 5: 5, 7 and 9 stand for themselves
    assert short[2].tolist() == [3, 5, 9, 7] and short[4] == 5 and short[5].tolist() == [1, CO.DEVICE_NONE, CO.DEVICE_NONE, CO.DEVICE_NONE]
    assert short[6].tolist() == [2, 1, 1, 1]
    assert _same(short, CO.collapse_by_loop((sc, ids), None, g[:5], 2, 4))


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_seeds_meet_their_conditions():
    """tests/test_gpu_collapse_fuzz.py asserts, on the device's own outputs, that at least half of its (case, query) pairs
    have collapsed < matches and that at least half have collapsed >= 2, for either entry (check_shares there). These are
    properties of the committed seeds: replayed here from the model, so that they are settled without a device. Both forms of
    collapse_best_kernel and both kinds of call are among the cases."""
    import test_gpu_collapse_fuzz as Y

    totals, lds_form, with_filter, kinds, past_the_map = [], 0, 0, set(), 0
    for seed, kind, ds, fs in Y.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = Y.Z.F.make_dictionary(r, kind, **ds), Y.Z.F.make_dictionary(r, kind, **fs)
        for i in range(Y.CASES_PER_DICTIONARY):
            case = Y.draw_collapse_case(Dd, Df, 100 * seed + i)
            totals.append(Y.model_shares(case))
            lds_form += case.n_groups <= 256
            with_filter += case.mask is not None
            past_the_map += len(case.group_of) < case.base.num_docs
            kinds.add(case.map_kind)
            assert 1 <= case.n_groups <= 600
    n = len(totals)
    assert n == 240 and kinds == set(FA.MAPS)
    assert n // 2 < lds_form < 5 * n // 6 and n // 3 < with_filter < 2 * n // 3 and past_the_map > n // 10
    Y.check_shares(np.sum(totals, axis=0))
    assert np.sum(totals, axis=0).tolist() == [[4800, 4167, 3612], [4800, 3075, 2528]]  # (the figures of that file's docstring)
