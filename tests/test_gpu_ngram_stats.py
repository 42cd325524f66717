"""The n-gram statistics on the GPU through the C ABI (dint_count_ngrams, dint_select_ngrams: include/dint_hip.h "block statistics
on the device") against the plain model of tests/ngram_stats.py, on its named cases and fuzz draws (which
tests/test_ngram_stats_cpu.py checks against the oracle, and checks to be what they are said to be): the counts with the position
of the FIRST occurrence, the pre-selection cut of top_k > 0 with its ties, the selection's order and per-context first top_k, the
saving filter at its boundary, the refusals. Every input is a few thousand integers at most; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import ngram_stats as NS
from dint_amd import host

pytestmark = pytest.mark.gpu

DINT_OK, DINT_ERR_ARG = 0, -1


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev

    return dev


@pytest.fixture(scope="module")
def up():
    """case -> its gaps on the device, uploaded once"""
    import torch

    made = {}

    def of(case):
        if case.name not in made:
            made[case.name] = torch.from_numpy(case.gaps.view(np.int32)).cuda()
        return made[case.name]

    return of


def _counted(device, up, case, top_k=0):
    """dint_count_ngrams' entries, checked to be distinct and clean"""
    entries, _ = device.count_ngrams(up(case), case.starts, case.multi, top_k=top_k)
    assert entries.dtype == NS.NGRAM_DTYPE and not entries["pad"].any(), case.name
    assert len(NS.as_set(entries)) == len(entries) == len({(int(e["ctx"]), case.ngram(e)) for e in entries}), case.name
    return entries


def _check_counts(device, up, case):
    want = NS.as_set(case.entries)
    got = _counted(device, up, case)
    assert NS.as_set(got) == want, case.name                           # (ctx, len, freq, pos): pos is the FIRST occurrence
    assert NS.as_set(_counted(device, up, case)) == want, case.name    # and again
    return got


def _kind(case):
    return host.MULTI_PACKED if case.multi else host.SINGLE_PACKED


# ---- counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NS.CASE_NAMES)
def test_counts_of_the_named_cases(device, up, name):
    case = NS.cases()[name]
    got = _check_counts(device, up, case)
    if name == "multi, no whole block":
        assert got.size == 0
    if name == "contexts":
        by = {(int(e["ctx"]), case.ngram(e)): int(e["freq"]) for e in got}
        for ctx in range(6):                                           # six separate entries, each with its context's count
            assert by[ctx, (0,)] == case.counts[ctx, (0,)][0] and by[ctx, (0, 0)] == case.counts[ctx, (0, 0)][0]
    if name == "first occurrence":
        by = {case.ngram(e): (int(e["freq"]), int(e["pos"])) for e in got}
        assert [by[g] for g in NS.FIRST_NGRAMS] == [(41, 255), (41, 254)]


def test_counts_of_the_fuzz_draws(device, up):
    for d in NS.draws():
        _check_counts(device, up, d)


# ---- the pre-selection cut ------------------------------------------------------------------------------------------------
def _check_cut(device, up, case, top_k):
    what = (case.name, top_k)
    everything = _counted(device, up, case)
    assert NS.as_set(everything) == NS.as_set(case.entries), what
    back = _counted(device, up, case, top_k=top_k)
    assert NS.as_set(back) == NS.as_set(NS.cut(case.entries, case.total, top_k)), what
    want = NS.as_list(NS.select(case.entries, case.gaps, case.total, top_k))
    assert NS.as_list(device.select_ngrams(up(case), back, case.total, top_k=top_k)) == want, what
    assert NS.as_list(device.select_ngrams(up(case), everything, case.total, top_k=top_k)) == want, what


def test_cut_of_the_fuzz_draws(device, up):
    for d in NS.draws():
        _check_cut(device, up, d, d.top_k)


@pytest.mark.parametrize("top_k", NS.TIE_TOP_KS)
def test_cut_at_ties(device, up, top_k):
    _check_cut(device, up, NS.cases()["ties"], top_k)


# ---- the selection --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ties", "gaps in contexts", "contexts"])
def test_selection_order_and_the_first_top_k_of_every_context(device, up, name):
    case = NS.cases()[name]
    entries = _counted(device, up, case)
    kept = NS.select(case.entries, case.gaps, case.total, 2**32 - 1)
    top_ks = {65536}
    for ctx in sorted(set(kept["ctx"].tolist())):
        n = int((kept["ctx"] == ctx).sum())
        top_ks |= {k for k in (1, n - 1, n, n + 1) if k > 0}
    assert len(top_ks) >= 5
    for top_k in sorted(top_ks):
        want = NS.select(case.entries, case.gaps, case.total, top_k)
        got = device.select_ngrams(up(case), entries, case.total, top_k=top_k)
        assert NS.as_list(got) == NS.as_list(want), (name, top_k)
        assert host.pack_dictionary(_kind(case), case.gaps, got) == host.pack_dictionary(_kind(case), case.gaps, want), (name, top_k)
        assert max(int((got["ctx"] == c).sum()) for c in set(got["ctx"].tolist())) <= top_k


# ---- the saving filter ----------------------------------------------------------------------------------------------------
def test_filter_at_its_boundary(device):
    """the totals of NS.FILTER_TOTALS (1e7 times 80, 176, 368 and 752, and one to either side) passed as total_ints over entries
    counted from 23 integers: n-grams of freq 1 leave at the total itself; the pair of freq 2 at 1.6e9; single integers never"""
    import torch

    gaps, starts, model = NS.boundary_collection()
    gaps_dev = torch.from_numpy(gaps.view(np.int32)).cuda()
    entries, _ = device.count_ngrams(gaps_dev, starts, False)
    assert NS.as_set(entries) == NS.as_set(model)
    sizes = {}
    for total in NS.FILTER_TOTALS + (2 * 80 * 10**7 - 1, 2 * 80 * 10**7, int(gaps.size), 10**15, 2**63):
        want = NS.select(model, gaps, total, 65536)
        got = device.select_ngrams(gaps_dev, entries, total, top_k=65536)
        assert NS.as_list(got) == NS.as_list(want), total
        assert int((got["len"] == 1).sum()) == 19, total               # 16 + 3 single integers survive every total
        sizes[total] = len(got)
    assert [sizes[80 * 10**7 + d] for d in (-1, 0, 1)] == [35, 27, 27]
    assert [sizes[176 * 10**7 + d] for d in (-1, 0, 1)] == [26, 22, 22]
    assert [sizes[368 * 10**7 + d] for d in (-1, 0, 1)] == [22, 20, 20]
    assert [sizes[752 * 10**7 + d] for d in (-1, 0, 1)] == [20, 19, 19]
    assert sizes[10**15] == sizes[2**63] == 19 and sizes[int(gaps.size)] == 35


def test_a_saving_equal_to_the_threshold_is_dropped(device):
    """NS.EXACT_TRIPLES (tests/test_ngram_stats_cpu.py derives them): the saving equals 0.0001 / 1000 in double — dropped; one
    integer less in the total — kept, and first in the order"""
    import torch

    gaps, _, model = NS.boundary_collection()
    gaps_dev = torch.from_numpy(gaps.view(np.int32)).cuda()
    for freq, length, total in NS.EXACT_TRIPLES:
        e = NS.with_freq(model, length, freq)
        got = device.select_ngrams(gaps_dev, e, total, top_k=65536)
        assert NS.as_list(got) == NS.as_list(NS.select(e, gaps, total, 65536)) and len(got) == 19 and (got["len"] == 1).all()
        more = device.select_ngrams(gaps_dev, e, total - 1, top_k=65536)
        assert NS.as_list(more) == NS.as_list(NS.select(e, gaps, total - 1, 65536)) and len(more) == 20
        assert (int(more[0]["freq"]), int(more[0]["len"])) == (freq, length)


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_select_refuses_bad_arguments(device, up):
    case = NS.cases()["ties"]
    lib, gaps_dev, n_ints = device._lib, up(case), case.gaps.size
    good = NS.as_list(NS.select(case.entries, case.gaps, case.total, 5))

    def call(entries, top_k=5, with_n=True):
        e = entries.copy()
        n = C.c_size_t(12345)
        status = lib.dint_select_ngrams(0, gaps_dev.data_ptr(), n_ints, case.total, e.ctypes.data, e.size, top_k,
                                        C.byref(n) if with_n else None)
        return status, e, n.value

    status, e, n = call(case.entries)
    assert status == DINT_OK and NS.as_list(e[:n]) == good
    status, e, n = call(case.entries, top_k=0)
    assert status == DINT_ERR_ARG and e.tobytes() == case.entries.tobytes()
    status, e, _ = call(case.entries, with_n=False)
    assert status == DINT_ERR_ARG and e.tobytes() == case.entries.tobytes()
    for field, value, length in (("len", 0, None), ("len", 17, None), ("ctx", 8, None), ("pos", n_ints, 1), ("pos", n_ints - 1, 2),
                                 ("pos", n_ints - 15, 16), ("pos", 2**63, 1), ("pos", 2**64 - 1, 2)):
        for at in (0, len(case.entries) - 1):                          # the first entry and the last
            bad = case.entries.copy()
            bad[field][at] = value
            if length is not None:
                bad["len"][at] = length
            status, e, n = call(bad)
            assert status == DINT_ERR_ARG and n == 0 and e.tobytes() == bad.tobytes(), (field, value, at)
    ok = case.entries.copy()                                           # the last integers of the collection are in bounds
    ok["pos"][0], ok["len"][0] = n_ints - 16, 16
    assert call(ok)[0] == DINT_OK
    status, e, n = call(case.entries)                                  # and the refusals left nothing behind
    assert status == DINT_OK and NS.as_list(e[:n]) == good


def test_count_refuses_bad_arguments(device, up):
    case = NS.cases()["ties"]
    lib, gaps_dev, n_ints = device._lib, up(case), case.gaps.size

    def call(starts, with_entries=True, multi=0, top_k=0):
        starts = np.ascontiguousarray(starts, dtype=np.uint64)
        out, n, ms = C.c_void_p(0xDEAD), C.c_size_t(12345), C.c_float()
        status = lib.dint_count_ngrams(0, multi, gaps_dev.data_ptr(), n_ints, starts.ctypes.data, len(starts) - 1, top_k,
                                       C.byref(out) if with_entries else None, C.byref(n), C.byref(ms))
        return status, out.value, n.value

    for multi in (0, 1):
        for top_k in (0, 3):
            assert call([0, 8, 4], multi=multi, top_k=top_k) == (DINT_ERR_ARG, None, 0)                  # descending
            assert call([0, 4, n_ints + 1], multi=multi, top_k=top_k) == (DINT_ERR_ARG, None, 0)         # an end past n_ints
            assert call([n_ints + 1, n_ints + 2], multi=multi, top_k=top_k) == (DINT_ERR_ARG, None, 0)   # a start past n_ints
            assert call([0, 300, 2**64 - 1], multi=multi, top_k=top_k) == (DINT_ERR_ARG, None, 0)
            assert call([0], multi=multi, top_k=top_k) == (DINT_OK, None, 0)                             # zero lists
    assert call(case.starts, with_entries=False)[0] == DINT_ERR_ARG
    status, out, n = call([0, n_ints, n_ints])                         # a list that ends at n_ints, and an empty one there
    assert status == DINT_OK and n > 0 and out
    lib.dint_free(C.c_void_p(out))
    none, _ = device.count_ngrams(gaps_dev, np.array([0], dtype=np.uint64), False)
    assert none.size == 0
    assert NS.as_set(_counted(device, up, case)) == NS.as_set(case.entries)
