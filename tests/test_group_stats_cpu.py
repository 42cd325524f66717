"""Per-group value statistics without a GPU: the two entries in the header, the library and the
binding, with DINT_ABI_VERSION still 6 and no new option; the argument errors that need no device; the model
(tests/group_stats.py) against a document-at-a-time loop on Python ints, on the named maps x the named columns and on the fuzz
draws; and the conditions that tests/test_gpu_group_stats_fuzz.py demands of its cases, from the model alone."""
import ctypes as C
import os

import numpy as np
import pytest

import facets as FA
import group_stats as GS
import ranked
from dint_amd import host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dint_ranked_or_group_stats_queries", "dint_ranked_and_group_stats_queries")
M32 = 0xFFFFFFFF
# the entries' arguments: the filtered call's up to filter (7), then facets, values, n_queries, counts, matches, scores, docids,
# group_stats, facet_counts, blocks_decoded, stream
N_ARGS = 7 + 11
OPTIONS = {"bundles", "index_concurrent", "query_lean_pages", "query_tail_pages", "query_fused_pages", "index_inline_tails", "chunk_split",
           "index_pair", "query_fused_copy", "query_batch_fused", "split_units", "refine_units"}


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert set(device.OPTIONS) == OPTIONS  # no new option
    assert "#define DINT_GROUP_STATS_MAX_RECORDS (1ull << 24)" in header
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert len(getattr(device._lib, name).argtypes) == N_ARGS
        declared = header[header.index(f"int {name}("):]
        assert declared[:declared.index(";")].count(",") + 1 == N_ARGS
        assert hasattr(device.QueryIndex, name[len("dint_"):])
    assert device._VALUE_STATS == GS.STATS_DTYPE and GS.STATS_DTYPE.itemsize == 24


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts, matches = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
    docids, rows = np.full(2048, 77, dtype=np.uint32), np.full(8, 77, dtype=np.uint32)
    scores = np.full(2048, -1.0, dtype=np.float32)
    recs = np.full(8, 77, dtype=GS.STATS_DTYPE)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: everything below is refused first)
    ok = dict(qi=fake, fd=fake, w=fake, k=10, cnt=counts, facets=fake, values=fake, recs=recs)
    cases = [dict(qi=None), dict(fd=None), dict(w=None), dict(cnt=None), dict(k=0), dict(k=1025), dict(facets=None), dict(values=None),
             dict(recs=None)]
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    for name in ENTRIES:
        for change in cases:
            a = dict(ok)
            a.update(change)
            assert getattr(lib, name)(a["qi"], a["fd"], a["w"], a["k"], terms.ctypes.data, offs.ctypes.data, None, a["facets"], a["values"], 1,
                                      ptr(a["cnt"]), matches.ctypes.data, scores.ctypes.data, docids.ctypes.data, ptr(a["recs"]),
                                      rows.ctypes.data, C.byref(blocks), None) == -1, (name, change)
    assert counts[0] == 77 and matches[0] == 77 and blocks.value == 77 and recs.tobytes() == np.full(8, 77, dtype=GS.STATS_DTYPE).tobytes()
    assert (docids == 77).all() and (rows == 77).all() and (scores == -1.0).all()


# ---- the model ----------------------------------------------------------------------------------------------------------
def _same(a, b, what=None):
    assert a.dtype == b.dtype == GS.STATS_DTYPE and a.shape == b.shape and a.tobytes() == b.tobytes(), what


def test_records_by_hand():
    sc = np.array([3.0, 2.0, 2.0, 1.0, 0.5, 0.25], dtype=np.float32)
    ids = np.array([0, 1, 2, 3, 4, 9], dtype=np.uint32)
    group_of = np.array([1, 1, FA.NONE, 0, 1, 2, 2, 2, 2, 2])
    values = np.array([4, M32, 6, 0, 7], dtype=np.uint32)  # (document 9 is in group 2 but past the column: it counts nowhere)
    got = GS.group_stats((sc, ids), None, group_of, 4, values)
    assert got.tolist() == [(1, 0, 0, 0), (3, 4 + M32 + 7, 4, M32), GS.EMPTY, GS.EMPTY]
    assert got[0].tolist() != GS.EMPTY  # n > 0 with min = max = 0 is not the empty record
    # a map shorter than the matches: document 4 and 9 are in no group
    assert GS.group_stats((sc, ids), None, group_of[:4], 2, values).tolist() == [(1, 0, 0, 0), (2, 4 + M32, 4, M32)]
    mask = np.array([True, False, True, True, False])
    assert GS.group_stats((sc, ids), mask, group_of, 2, values).tolist() == [(1, 0, 0, 0), (1, 4, 4, 4)]
    nothing = (np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint32))
    assert GS.group_stats(nothing, None, group_of, 3, values).tobytes() == GS.empty_records(1, 3).tobytes()
    out = GS.stacked([got, GS.group_stats(nothing, None, group_of, 4, values)], 4)
    assert out.shape == (2, 4) and out.dtype.itemsize == 24 and GS.stacked([], 4).shape == (0, 4)


def _small_index(r, num_docs):
    lists = [np.sort(r.choice(num_docs, int(r.integers(1, num_docs)), replace=False)).astype(np.uint32) for _ in range(5)]
    freqs = [r.integers(1, 4, x.size).astype(np.uint32) for x in lists]
    bounds = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)
    docids, fr = np.concatenate(lists), np.concatenate(freqs)
    return ranked.BuilderLists(docids, fr, bounds), ranked.norm_lens(host.sizes_from_postings(docids, fr, num_docs))


@pytest.mark.parametrize("n_groups", [1, 2, 7, 300])
def test_the_model_is_a_per_document_loop_on_the_named_cases(n_groups):
    r = np.random.default_rng(n_groups)
    num_docs = 700
    bl, nl = _small_index(r, num_docs)
    maps, cols = GS.named_maps(num_docs, n_groups), GS.named_columns(num_docs)
    assert set(FA.MAPS) < set(maps) and len(maps["short"]) < num_docs < len(maps["long"]) and set(GS.COLUMNS) <= set(cols)
    mask = r.random(num_docs // 2) < 0.5
    contributing = 0
    for conjunctive in (False, True):
        for q in ([0], [1, 2], [0, 1, 2, 3, 4], [3, 3, 4], []):
            every = GS.DF.every_match(bl, q, nl, num_docs, conjunctive)
            for m in (None, mask):
                ids = GS.matches_in(every, m).astype(np.int64)
                for map_name, group_of in maps.items():
                    row = FA.row_of(group_of, n_groups, ids)[0]
                    for col_name in GS.COLUMNS:
                        values = cols[col_name]
                        got = GS.group_stats(every, m, group_of, n_groups, values)
                        _same(got, GS.group_stats_by_loop(every, m, group_of, n_groups, values), (map_name, col_name, q))
                        assert (got["n"] <= row).all() and (len(values) < num_docs or np.array_equal(got["n"], row))
                        some = got["n"] > 0
                        assert (got["min"][some] <= got["max"][some]).all() and got[~some].tobytes() == GS.empty_records(1, int((~some).sum())).tobytes()
                        contributing += int(got["n"].sum())
    assert contributing > 10000


# ---- the fuzz's draws and conditions, from the model alone --------------------------------------------------------------
def test_the_fuzz_draws_are_the_loop_model_and_meet_their_conditions():
    """tests/test_gpu_group_stats_fuzz.py states six conditions on its cases (check_conditions there). They are properties of
    the committed seeds and the draws: replayed here from the model, so that they are settled without a device — and on every
    drawn case the numpy model equals the loop."""
    import test_gpu_group_stats_fuzz as P

    per_case, kinds = [], set()
    for spec in P.DICTIONARIES:
        seed, kind, ds, fs = spec
        r = np.random.default_rng(seed)
        Dd, Df = P.Z.F.make_dictionary(r, kind, **ds), P.Z.F.make_dictionary(r, kind, **fs)
        for s in P.seeds_of(spec):
            case = P.Y.draw_collapse_case(Dd, Df, s)
            map_kind, n_groups, group_of, col_kind, values = P.draws_of(case)
            assert 1 <= n_groups <= 600 and len(group_of) >= 1 and (np.asarray(group_of) < n_groups).all()
            every = P.every_of(case)
            model = P.model_of(case, every, n_groups, group_of, values)
            for entry, _ in P.ENTRIES:
                for m, got in zip(every[entry], model[entry]):
                    _same(got, GS.group_stats_by_loop(m, case.mask, group_of, n_groups, values), (s, entry))
            per_case.append(P.conditions_of(case, model, n_groups, group_of, values))
            kinds.add((map_kind, col_kind))
    assert len(per_case) == 36 and len(kinds) >= 10
    P.check_conditions(per_case)
