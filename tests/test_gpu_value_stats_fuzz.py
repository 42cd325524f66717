"""Differential fuzzing of the two value-stats ranked entries on the GPU, over the 240 cases of tests/test_gpu_collapse_fuzz.py
(draw_collapse_case, imported as tests/test_gpu_doc_values_fuzz.py imports it: seeded small indexes, a query mix, norm_lens, k,
option settings, a filter used in half of the cases). Per case one column and one edge set are drawn from a generator of the
case's own, np.random.default_rng([case seed, 0x57A7]) (tests/value_stats.py's draw_case), so the base draws do not shift: the
column as tests/doc_values.py's fuzz_values draws it (few distinct values, the whole u32 range, the docID, the docID reversed,
the lane d & 63; in half of the draws a 0 and a 0xFFFFFFFF planted), in a quarter of the cases cut below the index's docID space
and in a tenth two documents longer; the edges a count among 0 (0.1), 1-8 (0.3), 9-300 (0.35) and 1023 (0.25), taken a third each
from the column's present values, from their neighbours and uniformly. Both entries are held to the model
(tests/value_stats.py), record for record and row for row; their ranked outputs, matches and blocks_decoded to the filtered
entry's, bit for bit; and one query to the model asked alone. Every drawn case is checked; none is skipped.

Four conditions on the committed seeds keep the test from passing vacuously. They are properties of the draws, settled from the
model alone by tests/test_value_stats_cpu.py (check_shares) with the figures below. Of the 240 cases, per entry:
  - more than 256 buckets (the flush loop of the 256 threads takes more than one step): at least 1/6 — the count 1023 alone is
    drawn in a quarter of the cases;
  - a column shorter than the index's docID space (matches without a value): at least 1/6 — drawn in a quarter;
  - some query whose sum is at or above 2^32 (a 32-bit accumulator would wrap): at least 1/5 (OR) / 1/6 (AND) — the wide and
    the reversed columns are three tenths of the draws and two of their values already pass 2^32; a short column takes some away;
  - some query whose valued matches meet across pages (the atomics on the record and the row): OR, more than 256 valued
    matches, more than a page holds: at least 1/4 — a union of lists of up to 900 postings; AND, valued matches in two blocks of
    256 postings of the query's rarest list, which are two candidate pages: at least 1/10 — only the cases whose rarest lists
    are longer than a block can.
Reached by the committed seeds and these draws, from the model (240 cases an entry) — see FIGURES below, which
tests/test_value_stats_cpu.py asserts."""
from fractions import Fraction

import numpy as np
import pytest

import doc_filter as DF
import ranked
import test_gpu_collapse_fuzz as Y
import value_stats as VS

pytestmark = pytest.mark.gpu

Z = Y.Z
DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Y.DICTIONARIES, Y.CASES_PER_DICTIONARY, Y.ENTRIES

# per entry: (cases, more than 256 buckets, a short column, a sum at or above 2^32, matches that meet across pages)
FIGURES = {"or": (240, 70, 59, 78, 201), "and": (240, 70, 59, 78, 212)}
REQUIRED = {"or": (Fraction(1, 6), Fraction(1, 6), Fraction(1, 5), Fraction(1, 4)),
            "and": (Fraction(1, 6), Fraction(1, 6), Fraction(1, 6), Fraction(1, 10))}


def every_of(case):
    """-> {entry: per query every match of the unfiltered model}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    return {entry: [DF.every_match(lists, q, b.nl, b.num_docs, conjunctive) for q in b.qs] for entry, conjunctive in ENTRIES}


def draws_of(case):
    """-> (kind, values, which edge count, edges)"""
    return VS.draw_case(case.base.seed, case.base.num_docs)


def meets_across_pages(case, q, matches, values, conjunctive):
    """the fourth condition of one query: OR, more than 256 valued matches; AND, valued matches in two blocks of the rarest list"""
    ids = VS.matches_in(matches, case.mask)[1].astype(np.int64)
    ids = ids[ids < len(values)]
    if not conjunctive:
        return ids.size > 256
    X = case.base.X
    lens = np.diff(X.bounds.astype(np.int64))
    rarest = min(set(int(t) for t in q), key=lambda t: (int(lens[t]), t))
    own = X.docids[int(X.bounds[rarest]):int(X.bounds[rarest + 1])].astype(np.int64)
    return np.unique(np.searchsorted(own, ids) // 256).size >= 2


def shares_of(case, entry, conjunctive, per_query, every, values, n_edges):
    """one entry of one case -> (1, then whether the case meets each of the four conditions); per_query: the model's tuples"""
    c = VS.conditions(per_query, len(values), case.base.num_docs, n_edges)
    across = any(meets_across_pages(case, q, m, values, conjunctive) for q, m in zip(case.base.qs, every))
    return (1,) + tuple(int(x) for x in c[:3]) + (int(across),)


def model_of(case, every, values, edges):
    b = case.base
    return {entry: [VS.value_stats(m, case.mask, values, edges, b.k) for m in every[entry]] for entry, _ in ENTRIES}


def model_shares(case):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    every = every_of(case)
    _, values, _, edges = draws_of(case)
    model = model_of(case, every, values, edges)
    return [shares_of(case, e, c, model[e], every[e], values, len(edges)) for e, c in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the four conditions of this file's docstring"""
    for (entry, _), shares in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "cases, > 256 buckets, short column, sum >= 2^32, across pages:", shares)
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


def _bit_equal(got, want, what):
    for g, w in zip(got, want):
        if g is None or w is None:
            assert g is None and w is None, what
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def run_stats_case(device, dd, fd, Dd, Df, seed):
    case = Y.draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    kind, values, which, edges = draws_of(case)
    model = model_of(case, every, values, edges)
    col = device.DocValues(0, values)
    what = (seed, kind, len(values), b.num_docs, which, len(edges), case.mask is not None, b.k, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    shares = []
    for (entry, conjunctive), call, filtered in zip(ENTRIES, (qi.ranked_or_value_stats_queries, qi.ranked_and_value_stats_queries),
                                                    (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
        same = filtered(fd, wand, b.qs, f, k=b.k, with_stats=True)
        got = call(fd, wand, b.qs, col, edges=edges, filter=f, k=b.k, with_stats=True)
        _bit_equal(got[:4], same[:4], what + (entry, "the ranked outputs"))
        assert got[4] == same[4], what + (entry,)
        want = VS.stacked(model[entry], b.k, len(edges))
        _bit_equal(got[5:], want, what + (entry,))
        if got[6] is not None:
            assert np.array_equal(got[6].sum(axis=1, dtype=np.uint64), got[5]["n"]), what + (entry,)
        i = b.pick  # one query per call: its own answer
        one = call(fd, wand, [b.qs[i]], col, edges=edges, filter=f, k=b.k)
        _bit_equal(one[3:], VS.stacked([model[entry][i]], b.k, len(edges)), what + (entry, "alone"))
        shares.append(shares_of(case, entry, conjunctive, model[entry], every[entry], values, len(edges)))
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
    _TOTALS[seed] = np.sum([run_stats_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_value_stats_cases(device, spec):
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
