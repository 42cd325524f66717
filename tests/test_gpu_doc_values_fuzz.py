"""Differential fuzzing of the two sorted ranked entries and of the value-range filter on the GPU, over the 240 cases of
tests/test_gpu_collapse_fuzz.py (draw_collapse_case, imported as tests/test_gpu_paging_fuzz.py imports it: seeded small
indexes, a query mix, norm_lens, k, option settings, a filter used in half of the cases). Per case one column and one order,
and per (case, entry, query) one cursor, are drawn from a generator of the case's own, np.random.default_rng([case seed,
0x50A7]) (tests/doc_values.py's draw_case), so the base draws do not shift: the column is of few distinct values (0.4), the
whole u32 range (0.2), the docID (0.1), the docID reversed (0.1) or the lane d & 63 (0.2), in half of the draws with a 0 and a
0xFFFFFFFF planted; the cursor is with probability 0.7 a uniformly drawn match of the query under the case's mask, 0.1 a
match's value with a docID in [0, num_docs + 2), 0.1 none, 0.1 a random u32 value with such a docID; a query without a match
gets no draw. Both entries are held to the model (tests/doc_values.py), bit for bit, with and without the cursor; matches and
blocks_decoded to the filtered entry's; one query to the model asked alone; and the case's filter, rebuilt as the value range
[1, 1] over a second column v2 = mask, to the bitmap filter's info and answers.

Four conditions on the committed seeds keep the test from passing vacuously. They are asserted here on what the device
returns and replayed from the model alone by tests/test_doc_values_cpu.py (check_shares). Of each entry's 4800 (case, query)
pairs: the from-the-start page's docID set differs from the score-ranked call's top k in at least 2/5 (OR) / 1/5 (AND); the
value of hit k equals the value of the first match left out in at least 1/5 / 1/10; the cursor splits the matches
(0 < skipped < matches) in at least 1/2 / 1/2; a match with the cursor's value lies on each side of the cut in at least
1/5 / 1/5.
Reached by the committed seeds and these draws, from the model (4800 pairs an entry) — see FIGURES below, which
tests/test_doc_values_cpu.py asserts."""
from fractions import Fraction

import numpy as np
import pytest

import doc_filter as DF
import doc_values as DV
import ranked
import test_gpu_collapse_fuzz as Y

pytestmark = pytest.mark.gpu

Z = Y.Z
DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Y.DICTIONARIES, Y.CASES_PER_DICTIONARY, Y.ENTRIES

# per entry: (pairs, docID set differs, tie at the cut, cursor splits, the cursor's value on each side, matches > k)
FIGURES = {"or": (4800, 2225, 1319, 3504, 1622, 2246), "and": (4800, 1124, 628, 2653, 1147, 1154)}
REQUIRED = {"or": (Fraction(2, 5), Fraction(1, 5), Fraction(1, 2), Fraction(1, 5)),
            "and": (Fraction(1, 5), Fraction(1, 10), Fraction(1, 2), Fraction(1, 5))}


def every_of(case):
    """-> {entry: per query every match of the unfiltered model}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    return {entry: [DF.every_match(lists, q, b.nl, b.num_docs, conjunctive) for q in b.qs] for entry, conjunctive in ENTRIES}


def draws_of(case, every):
    """-> (kind, values, descending, {entry: per query a cursor})"""
    return DV.draw_case(case.base.seed, every, case.mask, case.base.num_docs)


def shares_of(every, mask, values, descending, cursors, k):
    """one entry's queries -> (pairs, then the pairs that meet each of DV.conditions' five)"""
    c = [DV.conditions(m, mask, values, descending, cur, k) for m, cur in zip(every, cursors)]
    return (len(c),) + tuple(sum(x[j] for x in c) for j in range(5))


def model_shares(case):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    every = every_of(case)
    _, values, descending, cursors = draws_of(case, every)
    return [shares_of(every[e], case.mask, values, descending, cursors[e], case.base.k) for e, _ in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the four conditions of this file's docstring"""
    for (entry, _), shares in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "pairs, differs, tie at the cut, splits, value on each side, matches > k:", shares)
        pairs = shares[0]
        assert pairs >= Z.QUERIES_PER_CASE * CASES_PER_DICTIONARY * len(DICTIONARIES)
        for got, need in zip(shares[1:5], REQUIRED[entry]):
            assert got >= need * pairs, (entry, shares, need)


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
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


def run_values_case(device, dd, fd, Dd, Df, seed):
    case = Y.draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    kind, values, descending, cursors = draws_of(case, every)
    col = device.DocValues(0, values)
    what = (seed, kind, descending, case.mask is not None, b.k, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    # the case's filter as a value range: v2 = mask, [1, 1]
    f2 = col2 = None
    if case.mask is not None:
        col2 = device.DocValues(0, case.mask.astype(np.uint32))
        f2 = qi.doc_filter_from_values(col2, 1, 1)
        i1, i2 = f.info, f2.info
        assert (i1.num_docs, i1.n_set, i1.n_blocks, i1.live_blocks) == (i2.num_docs, i2.n_set, i2.n_blocks, i2.live_blocks), what
    shares = []
    for (entry, _), sorted_call, filtered in zip(ENTRIES, (qi.ranked_or_sorted_queries, qi.ranked_and_sorted_queries),
                                                 (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
        after = cursors[entry]
        same = filtered(fd, wand, b.qs, f, k=b.k, with_stats=True)
        for cur in (after, None):
            per_q = cur if cur is not None else [None] * len(b.qs)
            want = DV.stacked([DV.sorted_page(m, case.mask, values, descending, c, b.k) for m, c in zip(every[entry], per_q)], b.k)
            got = sorted_call(fd, wand, b.qs, col, descending=descending, after=cur, filter=f, k=b.k, with_stats=True)
            _bit_equal(got[:5] + got[6:], want, what + (entry, cur is None))
            _bit_equal((got[4],), (same[3],), what + (entry,))
            assert got[5] == same[4], what + (entry,)
            if cur is not None:
                paged = got
            else:
                start = got
        i = b.pick  # one query per call: its own answer
        one = sorted_call(fd, wand, [b.qs[i]], col, descending=descending, after=[after[i]], filter=f, k=b.k)
        want = DV.stacked([DV.sorted_page(every[entry][i], case.mask, values, descending, after[i], b.k)], b.k)
        _bit_equal(one, [want[j] for j in (0, 1, 2, 3, 5)], what + (entry, "alone"))
        if f2 is not None:
            _bit_equal(filtered(fd, wand, b.qs, f2, k=b.k, with_stats=True)[:4], same[:4], what + (entry, "value range"))
            assert filtered(fd, wand, b.qs, f2, k=b.k, with_stats=True)[4] == same[4], what + (entry,)
            got2 = sorted_call(fd, wand, b.qs, col, descending=descending, after=after, filter=f2, k=b.k, with_stats=True)
            _bit_equal(got2[:5] + got2[6:], paged[:5] + paged[6:], what + (entry, "sorted under the value range"))
        # the conditions, from the device's outputs: the docID sets of the two orders, skipped and matches; the two about values
        # that a page does not return (what lies in front of the cut, and behind the page) from the MODEL's matches, which the
        # device's outputs have just been held to bit for bit — of the device it is required besides that hit k carries the tied
        # value and that a tied page begins with the cursor's value
        cond = [DV.conditions(m, case.mask, values, descending, c, b.k) for m, c in zip(every[entry], after)]
        differs = [set(start[2][q][:int(start[0][q])].tolist()) != set(same[2][q][:int(same[0][q])].tolist()) for q in range(len(b.qs))]
        assert differs == [c[0] for c in cond], what + (entry,)
        splits = [bool(0 < s < m) for s, m in zip(paged[6], paged[4])]
        assert splits == [c[2] for c in cond], what + (entry,)
        for q, c in enumerate(cond):
            assert not c[3] or int(paged[1][q, 0]) == after[q][0], what + (entry, q)
            assert c[4] == (int(start[4][q]) > b.k), what + (entry, q)
        shares.append((len(b.qs), sum(differs), sum(c[1] for c in cond), sum(splits), sum(c[3] for c in cond), sum(c[4] for c in cond)))
    for h in (f, f2, col2, col, qi, wand):
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
    _TOTALS[seed] = np.sum([run_values_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_values_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_draws_meet_their_conditions(device):
    """Over all the cases above: check_shares on what the device returned (a dictionary whose cases have not run in this
    session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    totals = np.sum([_TOTALS[spec[0]] for spec in DICTIONARIES], axis=0)
    check_shares(totals)
    assert [tuple(int(x) for x in t) for t in totals] == [FIGURES[e] for e, _ in ENTRIES]
