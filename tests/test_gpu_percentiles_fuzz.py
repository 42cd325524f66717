"""Differential fuzzing of the two percentile ranked entries on the GPU, over the 240 cases of tests/test_gpu_collapse_fuzz.py
(draw_collapse_case: seeded small indexes, a query mix, norm_lens, k, option settings, a filter used in half of the cases). Per
case the column is the one tests/test_gpu_value_stats_fuzz.py draws for it — the same np.random.default_rng([case seed, 0x57A7])
draw (tests/value_stats.py's draw_case), so that fuzz's measured coverage of columns carries over — and the percentile set comes
from a generator of its own, np.random.default_rng([case seed, 0x9C71]) (tests/percentiles.py's draw_percentiles): 1 to 16
entries, half of them common ranks (the ends, the quartiles, the tails) and half uniform over 0 .. 1000000, unsorted, repeats
possible, and in every third case (case seed % 3 == 0) 0 and 1000000 first. Both entries are held to the model
(tests/percentiles.py), count for count and value for value; their ranked outputs, matches and blocks_decoded to the filtered
entry's, bit for bit; the statistics to the value-stats model's; and one query to the model asked alone. Every drawn case is
checked; none is skipped.

Four conditions on the committed seeds keep the test from passing vacuously. They are properties of the draws, settled from the
model alone by tests/test_percentiles_cpu.py (check_shares) with the figures below. Of the 240 cases, per entry:
  - a column shorter than the index's docID space (matches without a value): at least 1/6 — drawn in a quarter;
  - some query with more than 256 valued matches, more than a page holds, so that pages meet in a counter row: at least 1/4 of
    the OR cases — a union of lists of up to 900 postings (the AND figure is recorded, nothing is demanded of it);
  - some query two of whose requested percentiles have different top bytes (the shared row of round 0 sends two selects of one
    query into different bins): at least 1/10;
  - some query whose requested percentile is a value that more than one of its matches holds (the remaining rank is not 0
    when the prefix is complete): at least 1/10.
Reached by the committed seeds and these draws, from the model (240 cases an entry) — see FIGURES below, which
tests/test_percentiles_cpu.py asserts: the last two are above 1/5."""
from fractions import Fraction

import numpy as np
import pytest

import percentiles as PC
import test_gpu_collapse_fuzz as Y
import test_gpu_value_stats_fuzz as S
import value_stats as VS

pytestmark = pytest.mark.gpu

Z = Y.Z
DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Y.DICTIONARIES, Y.CASES_PER_DICTIONARY, Y.ENTRIES

# per entry: (cases, a short column, more than 256 valued matches, two top bytes, a value held more than once)
FIGURES = {"or": (240, 59, 201, 55, 126), "and": (240, 59, 188, 54, 124)}
REQUIRED = {"or": (Fraction(1, 6), Fraction(1, 4), Fraction(1, 10), Fraction(1, 10)),
            "and": (Fraction(1, 6), Fraction(0), Fraction(1, 10), Fraction(1, 10))}

every_of = S.every_of


def draws_of(case):
    """-> (the column's kind, values, per_million)"""
    kind, values, _, _ = VS.draw_case(case.base.seed, case.base.num_docs)
    return kind, values, PC.draw_percentiles(case.base.seed)


def shares_of(case, matches, values, per_million):
    """one entry of one case -> (1, then whether the case meets each of the four conditions)"""
    return (1,) + tuple(int(x) for x in PC.conditions(matches, case.mask, values, per_million, case.base.num_docs))


def model_shares(case):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    every = every_of(case)
    _, values, per_million = draws_of(case)
    return [shares_of(case, every[e], values, per_million) for e, _ in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the four conditions of this file's docstring"""
    for (entry, _), shares in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "cases, short column, > 256 valued matches, two top bytes, a value held twice:", shares)
        cases = shares[0]
        assert cases >= CASES_PER_DICTIONARY * len(DICTIONARIES)
        for got, need in zip(shares[1:], REQUIRED[entry]):
            assert got >= need * cases, (entry, shares, need)


@pytest.fixture(scope="module")
def device():
    import torch

    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from dint_amd import device as dev

    return dev


@pytest.fixture(autouse=True)
def _options_back_to_default(device):
    yield
    device.reset_options()


_bit_equal = S._bit_equal


def run_percentile_case(device, dd, fd, Dd, Df, seed):
    case = Y.draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    kind, values, per_million = draws_of(case)
    col = device.DocValues(0, values)
    what = (seed, kind, len(values), b.num_docs, per_million, case.mask is not None, b.k, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    shares = []
    for (entry, _), call, filtered in zip(ENTRIES, (qi.ranked_or_percentile_queries, qi.ranked_and_percentile_queries),
                                          (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
        model = [PC.percentiles(m, case.mask, values, per_million) for m in every[entry]]
        same = filtered(fd, wand, b.qs, f, k=b.k, with_stats=True)
        got = call(fd, wand, b.qs, col, PC.percents(per_million), filter=f, k=b.k, with_stats=True)
        _bit_equal(got[:4], same[:4], what + (entry, "the ranked outputs"))
        assert got[4] == same[4], what + (entry,)
        _bit_equal(got[5:7], PC.stacked(model, len(per_million)), what + (entry,))
        stats = np.array([VS.value_stats(m, case.mask, values, None, 1)[0] for m in every[entry]], dtype=VS.STATS_DTYPE)
        _bit_equal(got[7:], (stats,), what + (entry, "the statistics"))
        i = b.pick  # one query per call, without the statistics: its own answer
        one = call(fd, wand, [b.qs[i]], col, PC.percents(per_million), filter=f, k=b.k)
        assert one[5] is None
        _bit_equal(one[3:5], PC.stacked([model[i]], len(per_million)), what + (entry, "alone"))
        shares.append(shares_of(case, every[entry], values, per_million))
    for h in (f, col, qi, wand):
        if h is not None:
            h.close()
    device.reset_options()
    return shares


_TOTALS = {}  # {dictionary seed: the shares summed over its cases, per entry}


def _run_dictionary(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    _TOTALS[seed] = np.sum([run_percentile_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_percentile_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_draws_meet_their_conditions(device):
    """Over all the cases above: check_shares on the cases the device has just been held to (a dictionary whose cases have not
    run in this session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    totals = np.sum([_TOTALS[spec[0]] for spec in DICTIONARIES], axis=0)
    check_shares(totals)
    assert [tuple(int(x) for x in t) for t in totals] == [FIGURES[e] for e, _ in ENTRIES]
