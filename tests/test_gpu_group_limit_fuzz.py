"""Differential fuzzing of the two group-limited ranked entries on the GPU: the 240 cases of tests/test_gpu_collapse_fuzz.py
(draw_collapse_case: a seeded small index, a query mix, norm_lens, k, option settings, a filter in half of the cases and ONE
group map of a random kind, n_groups in 1 .. 600, so both forms of collapse_max), each with a per_group of its own
(tests/group_limit.py's fuzz_per_group, a generator of its own per case: the case's base draws do not shift). Every output of
both entries is held to the model (tests/group_limit.py), bit for bit, matches, blocks_decoded and the rows to the faceted
entry's on the same arguments, and one query of every case is asked alone.

Conditions on the committed seeds keep the test from passing vacuously. They are asserted here on what the device returns
and replayed from the model alone by tests/test_group_limit_cpu.py (check_conditions), which holds the figures below
exactly. They are conditions, not measurements: counted on the CPU from the model with exactly this draw. Over the 4 800
(case, query) pairs of an entry:

    condition                                                            OR      AND     required
    kept < matches (some group was cut)                                  3 663   2 572   >= half
    a group's second or later match is kept                              3 567   2 635   >= half
    a group's places n and n + 1 hold equal scores (a tie across the cut) 1 563     976   >= one in ten

The draw gives 36 / 58 / 62 / 24 / 27 / 33 cases at per_group 1 / 2 / 3 / 4 / 8 / 16; each must be at least 20."""
import numpy as np
import pytest

import group_limit as GL
import ranked
import test_gpu_doc_filter_fuzz as Z
from test_gpu_collapse_fuzz import draw_collapse_case

pytestmark = pytest.mark.gpu

DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Z.DICTIONARIES, Z.CASES_PER_DICTIONARY, Z.ENTRIES


def every_of(case):
    """-> {entry: per query every_match's pair}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    return {entry: [GL.every_match(lists, q, b.nl, b.num_docs, conjunctive) for q in b.qs] for entry, conjunctive in ENTRIES}


def model_conditions(case, per_group):
    """-> per entry [or, and]: (pairs, the pairs with each of tests/group_limit.py's conditions), from the model alone"""
    every = every_of(case)
    out = []
    for entry, _ in ENTRIES:
        c = [GL.conditions(m, case.mask, case.group_of, per_group) for m in every[entry]]
        out.append((len(c),) + tuple(sum(x[j] for x in c) for j in range(3)))
    return out


def device_conditions(got, per_group):
    """the first two conditions from the arrays an entry returned with_stats and with_rows — (counts, scores, docids,
    matches, blocks, kept, hit_groups, hit_group_matches, hit_group_ranks, rows, skipped) -> (pairs, the pairs with kept <
    matches, the pairs where a group with two matches or more keeps its second: per_group >= 2 and a row entry >= 2). A tie
    across the cut lies between a kept and a cut document of one group; the cut one is in no output, so that condition is
    taken from the model once the outputs are bit-equal to it."""
    matches, kept, rows = got[3], got[5], got[9]
    cut = sum(int(c) < int(m) for m, c in zip(matches, kept))
    second = sum(bool(per_group >= 2 and row.size and int(row.max()) >= 2) for row in rows)
    return len(matches), cut, second


def check_conditions(per_entry, draws):
    """per_entry: model_conditions summed over the cases, [or, and]; draws: every case's per_group"""
    for (entry, _), (pairs, cut, second, tie) in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "pairs", pairs, "kept < matches", cut, "a second or later match kept", second, "a tie across the cut", tie)
        assert pairs >= Z.QUERIES_PER_CASE * CASES_PER_DICTIONARY * len(DICTIONARIES)
        assert 2 * cut >= pairs, (entry, cut, pairs)
        assert 2 * second >= pairs, (entry, second, pairs)
        assert 10 * tie >= pairs, (entry, tie, pairs)
    for n in (1, 2, 3, 4, 8, 16):
        assert list(draws).count(n) >= 20, (n, list(draws).count(n))


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
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), what


def run_case(device, dd, fd, Dd, Df, seed):
    """-> (per entry: (pairs, cut, second, tie) with cut and second from the device's outputs and tie from the model — the
    outputs are bit-equal to the model's by then —, per_group)"""
    case = draw_collapse_case(Dd, Df, seed)
    per_group = GL.fuzz_per_group(seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    facets = device.DocFacets(0, case.group_of, case.n_groups)
    what = (seed, case.map_kind, case.n_groups, len(case.group_of), case.mask is not None, b.k, per_group, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    out = []
    for (entry, _), fn, plain in zip(ENTRIES, (qi.ranked_or_group_limit_queries, qi.ranked_and_group_limit_queries),
                                     (qi.ranked_or_faceted_queries, qi.ranked_and_faceted_queries)):
        per_query = [GL.group_limit(m, case.mask, case.group_of, case.n_groups, b.k, per_group) for m in every[entry]]
        want = GL.stacked(per_query, b.k, case.n_groups)
        got = fn(fd, wand, b.qs, facets, per_group, filter=f, k=b.k, with_stats=True, with_rows=True)
        _bit_equal(got[:4] + got[5:], want, what + (entry,))
        same = plain(fd, wand, b.qs, facets, filter=f, k=b.k, with_stats=True)
        _bit_equal((got[3], got[9]), (same[3], same[5]), what + (entry,))
        assert got[4] == same[4], what + (entry,)
        i = b.pick  # one query per call, without the stats and the rows, behind its own third hit: its own answer
        cursor = (per_query[i][1][2], int(per_query[i][2][2])) if per_query[i][0] >= 3 else None
        alone = GL.group_limit(every[entry][i], case.mask, case.group_of, case.n_groups, b.k, per_group, cursor)
        one = fn(fd, wand, [b.qs[i]], facets, per_group, after=[cursor], filter=f, k=b.k)
        alone = GL.stacked([alone], b.k, case.n_groups)
        _bit_equal(one, [alone[j] for j in (0, 1, 2, 4, 5, 6, 7, 9)], what + (entry, "alone"))
        pairs, cut, second = device_conditions(got, per_group)
        model = [GL.conditions(m, case.mask, case.group_of, per_group) for m in every[entry]]
        assert cut == sum(c[0] for c in model) and second == sum(c[1] for c in model), what + (entry,)
        out.append((pairs, cut, second, sum(c[2] for c in model)))
    if f is not None:
        f.close()
    facets.close()
    qi.close()
    wand.close()
    device.reset_options()
    return out, per_group


_TOTALS = {}  # {dictionary seed: (the conditions summed over its cases, per entry; its cases' per_group)}


def _run_dictionary(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    ran = [run_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)]
    _TOTALS[seed] = (np.sum([x[0] for x in ran], axis=0), [x[1] for x in ran])


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_group_limit_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_limit_cuts_keeps_and_ties_enough(device):
    """Over all the cases above: check_conditions on what the device returned (a dictionary whose cases have not run in this
    session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    check_conditions(np.sum([_TOTALS[spec[0]][0] for spec in DICTIONARIES], axis=0),
                     [n for spec in DICTIONARIES for n in _TOTALS[spec[0]][1]])
