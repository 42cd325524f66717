"""Group-limited ranked queries without a GPU: the entries in the header, the library and the
binding, with DINT_ABI_VERSION still 6 and the option list unchanged; the argument errors that need no device; the model
(tests/group_limit.py) against a document-at-a-time loop, against tests/collapse.py's at per_group = 1 and against
tests/paging.py's where no group is cut; and the conditions that tests/test_gpu_group_limit_fuzz.py demands of its committed
seeds, from the model alone."""
import ctypes as C
import os

import numpy as np
import pytest

import collapse as CO
import facets as FA
import group_limit as GL
import paging as PG
import ranked
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dint_ranked_or_group_limit_queries", "dint_ranked_and_group_limit_queries")


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "#define DINT_GROUP_LIMIT_MAX 16" in header and device.GROUP_LIMIT_MAX == 16 == GL.MAX
    assert "8 BYTES PER (QUERY, GROUP, PLACE)" in " ".join(header.replace("*", " ").split())  # (the table's device memory is stated)
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert hasattr(device.QueryIndex, name[len("dint_"):])
        types = getattr(device._lib, name).argtypes
        assert len(types) == 23 and types[3] is C.c_uint32 and types[8] is C.c_uint32 and types[10] is C.c_size_t


def test_no_option_is_added():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    # the switches are the header's DINT_OPT_* before the workspace bound, twelve of them, and the bound is alone
    assert not [o for o in list(device.OPTIONS) + list(device.LIMITS) if "group" in o or "limit" in o]
    assert list(device.LIMITS) == ["query_or_pass_pages"] and len(device.OPTIONS) == 12
    names = [ln.split()[0].rstrip(",") for ln in header.split("typedef enum dint_option")[1].split("}")[0].splitlines()
             if ln.strip().startswith("DINT_OPT_")]
    switches = [n[len("DINT_OPT_"):].lower() for n in names if n not in ("DINT_OPT_COUNT_", "DINT_OPT_QUERY_OR_PASS_PAGES")]
    assert list(device.OPTIONS) == switches


def test_the_binding_refuses_a_per_group_out_of_range():
    from dint_amd import device

    qi = object.__new__(device.QueryIndex)  # (no handle: the refusals come before one is read)
    for fn in (qi.ranked_or_group_limit_queries, qi.ranked_and_group_limit_queries):
        for per_group in (0, 17, -1, 1 << 32):
            with pytest.raises(ValueError):
                fn(None, None, [[0]], None, per_group)
    for entry in ("or_group_limit", "and_group_limit"):
        with pytest.raises(ValueError):
            next(qi.ranked_pages(entry, None, None, [[0]], facets=object()))  # (no per_group)
        with pytest.raises(ValueError):
            next(qi.ranked_pages(entry, None, None, [[0]], per_group=2))  # (no facets)


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    out = {"counts": np.full(1, 77, dtype=np.uint64), "matches": np.full(1, 77, dtype=np.uint64), "kept": np.full(1, 77, dtype=np.uint64),
           "skipped": np.full(1, 77, dtype=np.uint64), "scores": np.full(2048, -1.0, dtype=np.float32),
           "docids": np.full(2048, 77, dtype=np.uint32), "hit_groups": np.full(2048, 77, dtype=np.uint32),
           "hit_group_matches": np.full(2048, 77, dtype=np.uint32), "hit_group_ranks": np.full(2048, 77, dtype=np.uint32),
           "rows": np.full(8, 77, dtype=np.uint32)}
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: what needs no handle is refused first)
    nan = np.array([(np.nan, 3)], dtype=[("score", "<f4"), ("docid", "<u4")])
    fine = np.array([(1.5, 3)], dtype=nan.dtype)

    def attempt(call, qi=fake, fd=fake, w=fake, k=10, facets=fake, per_group=2, after=None, n=1, null=()):
        p = {name: None if name in null else a.ctypes.data for name, a in out.items()}
        st = call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, facets, per_group, after.ctypes.data if after is not None else None, n,
                  p["counts"], p["matches"], p["kept"], p["skipped"], p["scores"], p["docids"], p["hit_groups"], p["hit_group_matches"],
                  p["hit_group_ranks"], p["rows"], C.byref(blocks), None)
        assert all((a == (-1.0 if name == "scores" else 77)).all() for name, a in out.items()) and blocks.value == 77  # nothing is written
        return st

    for name in ENTRIES:
        call = getattr(lib, name)
        for cursor in (None, fine):
            assert attempt(call, qi=None, after=cursor) == -1
            assert attempt(call, fd=None, after=cursor) == -1
            assert attempt(call, w=None, after=cursor) == -1
            assert attempt(call, facets=None, after=cursor) == -1
            for k in (0, 1025):
                assert attempt(call, k=k, after=cursor) == -1
            for per_group in (0, 17, 0xFFFFFFFF):
                assert attempt(call, per_group=per_group, after=cursor) == -1
            for required in ("counts", "scores", "kept", "hit_groups", "hit_group_matches", "hit_group_ranks"):
                assert attempt(call, null=(required,), after=cursor) == -1, required
                assert attempt(call, null=(required, "matches", "skipped", "docids", "rows"), after=cursor) == -1, required
        assert attempt(call, after=nan) == -1  # a NaN cursor
        # the record cap, with lying sizes: a map has at least one group, so n_queries * per_group just over 2^27 is refused
        # before an offset, a cursor or a handle is read
        for per_group in (1, 2, 16):
            assert attempt(call, per_group=per_group, n=(1 << 27) // per_group + 1) == -1


# ---- the model ----------------------------------------------------------------------------------------------------------
def _same(x, y):
    return len(x) == len(y) and all(
        np.asarray(a).dtype == np.asarray(b).dtype and np.asarray(a).tobytes() == np.asarray(b).tobytes() if isinstance(a, np.ndarray)
        else a == b for a, b in zip(x, y))


def _collection(seed):
    r = np.random.default_rng(seed)
    num_docs = int(r.integers(30, 400))
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 4, x.size).astype(np.uint32) for x in lists]  # (few distinct freqs: equal scores occur)
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    nl = np.ones(num_docs, dtype=np.float32) if seed % 2 else ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))
    return r, num_docs, ranked.BuilderLists(docids, fr, bounds), nl


@pytest.mark.parametrize("seed", range(6))
def test_the_model_is_a_per_document_loop(seed):
    r, num_docs, bl, nl = _collection(seed)
    cut = second = ties = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], [2, 0], []):
            every = GL.every_match(bl, q, nl, num_docs, conjunctive)
            for n_mask in (None, num_docs, num_docs // 2):
                mask = None if n_mask is None else r.random(n_mask) < 0.5
                sc, ids = PG.in_filter(every, mask)
                cursors = [None, (0.0, 0), (np.inf, 5)]
                if ids.size:
                    i = int(r.integers(0, ids.size))
                    cursors += [(sc[i], int(ids[i])), (sc[i], int(r.integers(0, num_docs + 2))), (sc[i] * np.float32(0.75), 0)]
                for name in FA.MAPS:
                    for n_map, n_groups in ((num_docs, 3), (num_docs // 2, 17), (num_docs + 9, 300)):  # the map: at, below, above
                        g = FA.named_map(name, n_map, n_groups, seed=seed)
                        per_group = int(r.choice(GL.PER_GROUP_CHOICES))
                        for k, after in ((1, cursors[0]), (10, cursors[int(r.integers(0, len(cursors)))]), (1000, cursors[-1])):
                            got = GL.group_limit(every, mask, g, n_groups, k, per_group, after)
                            assert _same(got, GL.group_limit_by_loop(every, mask, g, n_groups, k, per_group, after)), (q, name, n_map, k, after)
                            count, scores, hit_ids, matches, kept, hit_groups, hit_matches, hit_ranks, row, skipped = got
                            assert count == min(kept - skipped, k) and skipped <= kept <= matches == ids.size
                            assert np.array_equal(row, FA.row_of(g, n_groups, ids)[0])
                            # what is kept: min(per_group, matches) of every group, and every match in no group
                            assert kept == int(np.minimum(row, per_group).sum()) + matches - int(row.sum())
                            shown = hit_groups[:count]
                            grouped = shown != GL.DEVICE_NONE
                            assert (hit_ranks[:count] < per_group).all() and not hit_ranks[count:].any() and not hit_ranks[:count][~grouped].any()
                            assert (hit_ranks[:count][grouped] < row[shown[grouped]]).all()
                            pairs = list(zip(shown[grouped].tolist(), hit_ranks[:count][grouped].tolist()))
                            assert len(set(pairs)) == len(pairs)  # a place of a group is shown once
                            assert np.array_equal(hit_matches[:count][grouped], row[shown[grouped]])
                            assert (hit_matches[:count][~grouped] == 1).all() and not hit_matches[count:].any()
                            assert (np.diff(scores[:count]) <= 0).all()
                            cut += kept < matches
                            second += bool((hit_ranks[:count] >= 1).any())
                ties += int(sc.size - np.unique(sc).size)
    assert cut > 100 and second > 100 and ties > 0


@pytest.mark.parametrize("seed", range(4))
def test_per_group_of_one_is_the_collapse_and_a_large_one_the_page(seed):
    """per_group = 1 is tests/collapse.py's collapse behind tests/paging.py's cursor, with every rank 0; a per_group of at
    least the largest group's matches cuts no group, and the hits are tests/paging.py's page."""
    r, num_docs, bl, nl = _collection(seed)
    uncut = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], []):
            every = GL.every_match(bl, q, nl, num_docs, conjunctive)
            for mask in (None, r.random(num_docs) < 0.5):
                sc, ids = PG.in_filter(every, mask)
                cursors = [None] + ([(sc[ids.size // 2], int(ids[ids.size // 2])), (sc[0], num_docs)] if ids.size else [])
                for name in FA.MAPS:
                    for n_map, n_groups in ((num_docs, 3), (num_docs // 2, 17), (num_docs + 9, 300)):
                        g = FA.named_map(name, n_map, n_groups, seed=seed)
                        for after in cursors:
                            for k in (1, 10, 1000):
                                one = GL.group_limit(every, mask, g, n_groups, k, 1, after)
                                assert not one[7].any()
                                assert _same(one[:7] + one[8:], PG.collapsed_page_after(every, mask, g, n_groups, after, k)), (q, name, k, after)
                                row = one[8]
                                if int(row.max(initial=0)) > GL.MAX:
                                    continue
                                wide = GL.group_limit(every, mask, g, n_groups, k, max(1, int(row.max(initial=0))), after)
                                page = PG.page_after(every, mask, after, k)
                                assert _same((wide[0], wide[1], wide[2], wide[3], wide[9]), page), (q, name, k, after)
                                assert wide[4] == wide[3]
                                uncut += 1
    assert uncut > 100


def test_equal_scores_go_to_the_smaller_docid_at_the_cut():
    sc = np.array([1.0, 2.0, 2.0, 2.0, 0.5, 2.0, 2.0], dtype=np.float32)
    ids = np.array([7, 9, 3, 5, 1, 4, 8], dtype=np.uint32)
    g = np.array([0, 0, 0, 1, 1, 1, 1, 1, 1, 1], dtype=np.int64)  # 3, 4, 5, 7, 8, 9 -> 1; 1 -> 0
    # group 1 in key order: 3, 4, 5, 8, 9 (all 2.0), then 7 (1.0): the cut falls between equal scores for per_group 1 .. 4
    for per_group, want in ((1, [3, 1]), (2, [3, 4, 1]), (3, [3, 4, 5, 1]), (4, [3, 4, 5, 8, 1]), (5, [3, 4, 5, 8, 9, 1]), (6, [3, 4, 5, 8, 9, 7, 1]),
                            (16, [3, 4, 5, 8, 9, 7, 1])):
        got = GL.group_limit((sc, ids), None, g, 2, 8, per_group)
        n = len(want)
        assert got[0] == n == got[4] and got[2][:n].tolist() == want and (got[2][n:] == 0xFFFFFFFF).all(), per_group
        assert got[7][:n].tolist() == list(range(n - 1)) + [0] and got[6][:n].tolist() == [6] * (n - 1) + [1]
        assert got[5][:n].tolist() == [1] * (n - 1) + [0] and got[3] == 7 and got[8].tolist() == [1, 6] and got[9] == 0
        assert GL.conditions((sc, ids), None, g, per_group) == (per_group < 6, per_group > 1, per_group < 5)
        assert _same(got, GL.group_limit_by_loop((sc, ids), None, g, 2, 8, per_group))
    # a cursor at the group's second place: what lies after it starts at the third, and skipped counts the kept before
    got = GL.group_limit((sc, ids), None, g, 2, 2, 3, after=(2.0, 4))
    assert got[0] == 2 and got[2].tolist() == [5, 1] and got[7].tolist() == [2, 0] and got[9] == 2 and got[4] == 4
    # a cursor at a document that was cut: it need not be kept, the cut is on the keys
    got = GL.group_limit((sc, ids), None, g, 2, 4, 2, after=(2.0, 8))
    assert got[0] == 1 and got[2][0] == 1 and got[9] == 2 and got[4] == 3
    short = GL.group_limit((sc, ids), None, g[:5], 2, 8, 1)  # the map ends at 5: 5, 7, 8 and 9 stand for themselves
    assert short[2][:short[0]].tolist() == [3, 5, 8, 9, 7, 1] and short[4] == 6 and short[7].tolist() == [0] * 8
    assert short[5][:6].tolist() == [1, GL.DEVICE_NONE, GL.DEVICE_NONE, GL.DEVICE_NONE, GL.DEVICE_NONE, 0]


def test_the_per_group_draw():
    assert [GL.fuzz_per_group(s) for s in range(3)] == [int(np.random.default_rng([s, 0x61C7]).choice((1, 2, 2, 3, 3, 4, 8, 16))) for s in range(3)]
    assert set(GL.PER_GROUP_CHOICES) == {1, 2, 3, 4, 8, 16}


# ---- the fuzz's conditions, from the model alone ------------------------------------------------------------------------
def test_the_fuzz_seeds_meet_their_conditions():
    """tests/test_gpu_group_limit_fuzz.py asserts its conditions on the device's own outputs (check_conditions there). They
    are properties of the committed seeds: replayed here from the model, so that they are settled without a device, and
    held to the figures of that file's docstring exactly."""
    import test_gpu_group_limit_fuzz as Y

    totals, draws = [], []
    for seed, kind, ds, fs in Y.DICTIONARIES:
        r = np.random.default_rng(seed)
        Dd, Df = Y.Z.F.make_dictionary(r, kind, **ds), Y.Z.F.make_dictionary(r, kind, **fs)
        for i in range(Y.CASES_PER_DICTIONARY):
            case = Y.draw_collapse_case(Dd, Df, 100 * seed + i)
            per_group = GL.fuzz_per_group(100 * seed + i)
            draws.append(per_group)
            totals.append(Y.model_conditions(case, per_group))
    assert len(totals) == 240
    Y.check_conditions(np.sum(totals, axis=0), draws)
    assert [draws.count(n) for n in (1, 2, 3, 4, 8, 16)] == [36, 58, 62, 24, 27, 33]
    assert np.sum(totals, axis=0).tolist() == [[4800, 3663, 3567, 1563], [4800, 2572, 2635, 976]]
