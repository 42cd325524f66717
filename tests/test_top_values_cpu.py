"""Top values and distinct counts without a GPU: the two entries in the header, the library and the
binding, with DINT_ABI_VERSION still 6 and the options unchanged; the argument errors that need no device; and the model
(tests/top_values.py: np.unique and a lexsort) against a document-at-a-time loop with a dict on Python ints — on the named
columns, on the fuzz's draws, on ties, with n_top above the distinct count and on an empty column."""
import ctypes as C
import os

import numpy as np
import pytest

import top_values as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("dint_ranked_or_top_values_queries", "dint_ranked_and_top_values_queries")
M32 = 0xFFFFFFFF
# the entries' arguments: the filtered call's up to filter (7), then values, n_top, n_queries, counts, matches, scores, docids,
# value_counts, distinct_counts, top_n, top_values, top_counts, blocks_decoded, stream
N_ARGS = 7 + 14
OPTIONS = {"bundles", "index_concurrent", "query_lean_pages", "query_tail_pages", "query_fused_pages", "index_inline_tails", "chunk_split",
           "index_pair", "query_fused_copy", "query_batch_fused", "split_units", "refine_units"}


def _every(ids):
    ids = np.asarray(ids, dtype=np.uint32)
    return np.ones(ids.size, dtype=np.float32), ids


def _same(a, b, what=None):
    assert a[:3] == b[:3], (what, a[:3], b[:3])
    for x, y in zip(a[3:], b[3:]):
        assert x.dtype == y.dtype == np.uint32 and x.tobytes() == y.tobytes(), what


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "#define DINT_TOP_VALUES_MAX 1024u" in header and "#define DINT_RANKED_MAX_K 1024 " in header
    assert device.TOP_VALUES_MAX == TV.MAX_TOP == 1024
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert len(getattr(device._lib, name).argtypes) == N_ARGS == 21
        declared = header[header.index(f"int {name}("):]
        assert declared[:declared.index(";")].count(",") + 1 == N_ARGS
    assert hasattr(device.QueryIndex, "ranked_or_top_values_queries") and hasattr(device.QueryIndex, "ranked_and_top_values_queries")
    assert set(device.OPTIONS) == OPTIONS  # no new option


def test_argument_errors_need_no_device():
    from dint_amd import device

    lib = device._lib
    counts, matches = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64)
    vc, dc, tn = np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint64), np.full(1, 77, dtype=np.uint32)
    docids, tv, tc = np.full(2048, 77, dtype=np.uint32), np.full(2048, 77, dtype=np.uint32), np.full(2048, 77, dtype=np.uint32)
    scores = np.full(2048, -1.0, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: everything below is refused first)
    ok = dict(qi=fake, fd=fake, w=fake, k=10, cnt=counts, values=fake, n_top=10, vc=vc, dc=dc, tn=tn, tv=tv, tc=tc)
    cases = [dict(qi=None), dict(fd=None), dict(w=None), dict(cnt=None), dict(k=0), dict(k=1025), dict(values=None), dict(n_top=1025),
             dict(n_top=M32), dict(vc=None), dict(dc=None), dict(tn=None), dict(tv=None), dict(tc=None), dict(n_top=1, tv=None),
             dict(n_top=0, qi=None), dict(n_top=0, values=None, tv=None, tc=None)]
    ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
    for name in ENTRIES:
        for change in cases:
            a = dict(ok)
            a.update(change)
            st = getattr(lib, name)(a["qi"], a["fd"], a["w"], a["k"], terms.ctypes.data, offs.ctypes.data, None, a["values"], a["n_top"], 1,
                                    ptr(a["cnt"]), matches.ctypes.data, scores.ctypes.data, docids.ctypes.data, ptr(a["vc"]), ptr(a["dc"]),
                                    ptr(a["tn"]), ptr(a["tv"]), ptr(a["tc"]), C.byref(blocks), None)
            assert st == -1, (name, change)
    assert counts[0] == 77 and matches[0] == 77 and vc[0] == 77 and dc[0] == 77 and tn[0] == 77 and blocks.value == 77
    assert (docids == 77).all() and (tv == 77).all() and (tc == 77).all() and (scores == -1.0).all()


# ---- the model ----------------------------------------------------------------------------------------------------------
def test_top_values_by_hand():
    ids = [0, 1, 2, 3, 4, 5, 6, 9]
    values = np.array([40, 10, 30, M32, 10, 0, 30, 7, 7], dtype=np.uint32)  # (document 9 is past the column: no value)
    n, distinct, top_n, v, c = TV.top_values(_every(ids), None, values, 3)
    # counts: 10 -> 2, 30 -> 2, then 0, 40 and M32 once each: ties go to the smaller value
    assert (n, distinct, top_n) == (7, 5, 3) and v.tolist() == [10, 30, 0] and c.tolist() == [2, 2, 1]
    n, distinct, top_n, v, c = TV.top_values(_every(ids), None, values, 8)  # n_top above the distinct count: zeros past top_n
    assert (n, distinct, top_n) == (7, 5, 5) and v.tolist() == [10, 30, 0, 40, M32, 0, 0, 0] and c.tolist() == [2, 2, 1, 1, 1, 0, 0, 0]
    n, distinct, top_n, v, c = TV.top_values(_every(ids), None, values, 0)
    assert (n, distinct, top_n) == (7, 5, 0) and v.size == 0 and c.size == 0
    mask = np.array([True, False, True, False, False, False, True] + [True] * 3)
    assert TV.top_values(_every(ids), mask, values, 2)[:3] == (3, 2, 2)
    assert TV.top_values(_every(ids), mask, values, 2)[3].tolist() == [30, 40]
    for n_top in (0, 1, 4):  # an empty column, and no match at all
        for got in (TV.top_values(_every(ids), None, np.zeros(0, dtype=np.uint32), n_top), TV.top_values(_every([]), None, values, n_top)):
            assert got[:3] == (0, 0, 0) and not got[3].any() and not got[4].any() and got[3].size == n_top
    s = TV.stacked([TV.top_values(_every(ids), None, values, 2), TV.top_values(_every([]), None, values, 2)], 2)
    assert [x.dtype for x in s] == [np.uint64, np.uint64, np.uint32, np.uint32, np.uint32]
    assert s[0].tolist() == [7, 0] and s[1].tolist() == [5, 0] and s[2].tolist() == [2, 0] and s[3].tolist() == [[10, 30], [0, 0]]
    assert TV.stacked([], 3)[3].shape == (0, 3) and TV.stacked([TV.top_values(_every(ids), None, values, 0)], 0)[4].shape == (1, 0)


def test_the_named_columns_are_what_they_are_said_to_be():
    top = 9000
    cols = TV.named_columns(top)
    assert set(cols) == {"all equal", "v = d", "d % 7", "d // 100", "d % 1000", "0 and ones", "wide", "half", "empty"}
    assert np.unique(cols["all equal"]).size == 1 and np.unique(cols["v = d"]).size == top
    assert (np.diff(cols["d % 7"].astype(np.int64)) != 0).all()  # no two neighbours equal
    assert set(np.unique(cols["0 and ones"]).tolist()) == {0, M32} and cols["half"].size == top // 2 and cols["empty"].size == 0
    every = _every(np.arange(top))
    n, distinct, top_n, v, c = TV.top_values(every, None, cols["d % 1000"], 1024)
    assert (n, distinct, top_n) == (top, 1000, 1000) and (c[:1000] == 9).all() and v[:1000].tolist() == list(range(1000))
    n, distinct, top_n, v, c = TV.top_values(every, None, cols["v = d"], 257)
    assert distinct == top and (c == 1).all() and v.tolist() == list(range(257))
    assert TV.top_values(every, None, cols["0 and ones"], 3)[3:][0].tolist() == [0, M32, 0]


@pytest.mark.parametrize("name", list(TV.named_columns(10)))
def test_the_two_forms_agree_on_the_named_columns(name):
    top = 3000
    values = TV.named_columns(top)[name]
    r = np.random.default_rng(5)
    mask = r.random(top) < 0.6
    for ids in (np.arange(top), np.arange(0, top, 2), np.array([10, 20, 30, 40]), np.zeros(0, dtype=np.uint32)):
        for n_top in TV.N_TOPS:
            for m in (None, mask):
                _same(TV.top_values(_every(ids), m, values, n_top), TV.top_values_by_loop(_every(ids), m, values, n_top), (name, n_top))


def test_the_two_forms_agree_on_the_draws():
    kinds, tops = set(), set()
    for seed in range(60):
        num_docs = 1 + 37 * seed
        kind, values, n_top = TV.draw_case(seed, num_docs)
        assert values.dtype == np.uint32 and values.size <= num_docs and 0 <= n_top <= TV.MAX_TOP
        if kind == "all distinct":
            assert np.unique(values).size == values.size
        kinds.add(kind)
        tops.add(n_top)
        r = np.random.default_rng(seed)
        ids = np.flatnonzero(r.random(num_docs + 5) < 0.7)
        mask = r.random(num_docs + 5) < 0.5 if seed % 2 else None
        _same(TV.top_values(_every(ids), mask, values, n_top), TV.top_values_by_loop(_every(ids), mask, values, n_top), seed)
        again = TV.draw_case(seed, num_docs)
        assert again[0] == kind and again[2] == n_top and again[1].tobytes() == values.tobytes()
    assert kinds == set(TV.KINDS) and 0 in tops and 1024 in tops and tops & {255, 256, 257, 258} and tops & {511, 512, 513}


# ---- the fuzz's coverage, from the model alone --------------------------------------------------------------------------
def test_the_fuzz_cases_cover_their_ground():
    """tests/test_gpu_top_values_fuzz.py runs a handful of cases. What they cover is a property of the committed seeds and the
    draws: replayed here from the model, so that it is settled without a device."""
    import test_gpu_top_values_fuzz as T

    seen = []
    for spec in T.DICTIONARIES:
        seed, kind, ds, fs = spec
        r = np.random.default_rng(seed)
        Dd, Df = T.Z.F.make_dictionary(r, kind, **ds), T.Z.F.make_dictionary(r, kind, **fs)
        seen += [T.coverage_of(T.Y.draw_collapse_case(Dd, Df, s)) for s in T.case_seeds(spec)]
    assert len(seen) == T.CASES * len(T.DICTIONARIES) >= 30
    assert {c[0] for c in seen} == set(TV.KINDS) and any(c[1] for c in seen) and not all(c[1] for c in seen)
    tops = [c[2] for c in seen]
    assert 0 in tops and any(1 <= t <= 12 for t in tops) and any(t >= 256 for t in tops)
    assert sum(c[3] for c in seen) >= 5 and sum(c[4] for c in seen) >= 10
