"""Differential fuzzing of the two group-stats ranked entries on the GPU, over the first CASES_PER_DICTIONARY cases of every
dictionary of tests/test_gpu_collapse_fuzz.py (draw_collapse_case, as tests/test_gpu_value_stats_fuzz.py takes them: seeded small
indexes, a query mix, norm_lens, k, option settings, a filter used in half of the cases) — 36 cases, a few seconds in all. Per
case one map and one column are drawn from a generator of the case's own, np.random.default_rng([case seed, 0x6A57])
(tests/group_stats.py's draw_case), so the base draws do not shift: the map as tests/facets.py's fuzz_map draws it (1 .. 600
groups, both forms of group_stats_kernel; a map that ends below, at or above the index's docID space; in a quarter of the cases
at most 3 groups, so that a group gathers more than a page of matches), the column as tests/doc_values.py's fuzz_values draws it,
in a quarter of the cases cut below the index's docID space and in a tenth two documents longer. Both entries are held to the
model (tests/group_stats.py), record for record; their ranked outputs, matches and blocks_decoded to the filtered entry's and
their rows to the faceted entry's, bit for bit; and one query to the model asked alone. Every drawn case is checked; none is
skipped.

Six conditions keep the test from passing vacuously (tests/group_stats.py's CONDITIONS): across the cases, for each entry, each
must occur at least once — more than 256 groups and at most 256; a short column and a short map; a (query, group) sum at or above
2^32 (a 32-bit accumulator would wrap); a (query, group) with more than 256 contributing matches (more than a page holds: the
record meets across pages). They are properties of the committed seeds and the draws, settled from the model alone by
tests/test_group_stats_cpu.py (check_conditions), and asserted here again on the cases the device was held to."""
import numpy as np
import pytest

import doc_filter as DF
import group_stats as GS
import ranked
import test_gpu_collapse_fuzz as Y

pytestmark = pytest.mark.gpu

Z = Y.Z
DICTIONARIES, ENTRIES = Y.DICTIONARIES, Y.ENTRIES
CASES_PER_DICTIONARY = 6


def seeds_of(spec):
    return [100 * spec[0] + i for i in range(CASES_PER_DICTIONARY)]


def every_of(case):
    """-> {entry: per query every match of the unfiltered model}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    return {entry: [DF.every_match(lists, q, b.nl, b.num_docs, conjunctive) for q in b.qs] for entry, conjunctive in ENTRIES}


def draws_of(case):
    """-> (map kind, n_groups, group_of, column kind, values)"""
    return GS.draw_case(case.base.seed, case.base.num_docs)


def model_of(case, every, n_groups, group_of, values):
    return {entry: [GS.group_stats(m, case.mask, group_of, n_groups, values) for m in every[entry]] for entry, _ in ENTRIES}


def conditions_of(case, model, n_groups, group_of, values):
    """-> per entry [or, and] the case's GS.conditions"""
    return [GS.conditions(model[e], n_groups, len(group_of), len(values), case.base.num_docs) for e, _ in ENTRIES]


def model_conditions(case):
    """conditions_of, from the model alone"""
    _, n_groups, group_of, _, values = draws_of(case)
    return conditions_of(case, model_of(case, every_of(case), n_groups, group_of, values), n_groups, group_of, values)


def check_conditions(per_case):
    """per_case: conditions_of of every case — each condition occurs at least once for each entry"""
    seen = np.sum(np.array(per_case, dtype=np.int64), axis=0)  # [entry, condition]
    assert len(per_case) == CASES_PER_DICTIONARY * len(DICTIONARIES)
    for (entry, _), row in zip(ENTRIES, seen):
        print(entry, dict(zip(GS.CONDITIONS, row.tolist())))
        assert (row > 0).all(), (entry, dict(zip(GS.CONDITIONS, row.tolist())))


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
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), what


def run_group_stats_case(device, dd, fd, Dd, Df, seed):
    case = Y.draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    map_kind, n_groups, group_of, col_kind, values = draws_of(case)
    model = model_of(case, every, n_groups, group_of, values)
    facets, col = device.DocFacets(0, group_of, n_groups), device.DocValues(0, values)
    what = (seed, map_kind, n_groups, len(group_of), col_kind, len(values), b.num_docs, case.mask is not None, b.k, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    for (entry, _), call, filtered, faceted in zip(ENTRIES, (qi.ranked_or_group_stats_queries, qi.ranked_and_group_stats_queries),
                                                   (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries),
                                                   (qi.ranked_or_faceted_queries, qi.ranked_and_faceted_queries)):
        same = filtered(fd, wand, b.qs, f, k=b.k, with_stats=True)
        rows = faceted(fd, wand, b.qs, facets, filter=f, k=b.k, with_stats=True)[5]
        got = call(fd, wand, b.qs, facets, col, filter=f, k=b.k, with_facet_counts=True)
        _bit_equal(got[:4], same[:4], what + (entry, "the ranked outputs"))
        assert got[4] == same[4], what + (entry,)
        _bit_equal((got[5], got[6]), (GS.stacked(model[entry], n_groups), rows), what + (entry,))
        assert (got[5]["n"] <= got[6]).all(), what + (entry,)
        i = b.pick  # one query per call, without the rows: its own answer
        one = call(fd, wand, [b.qs[i]], facets, col, filter=f, k=b.k)
        assert one[6] is None
        _bit_equal((one[5],), (GS.stacked([model[entry][i]], n_groups),), what + (entry, "alone"))
    for h in (f, col, facets, qi, wand):
        if h is not None:
            h.close()
    device.reset_options()
    return conditions_of(case, model, n_groups, group_of, values)


_SEEN = {}  # {dictionary seed: conditions_of of its cases}


def _run_dictionary(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    _SEEN[seed] = [run_group_stats_case(device, dd, fd, Dd, Df, s) for s in seeds_of(spec)]


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_group_stats_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_draws_meet_their_conditions(device):
    """Over all the cases above: check_conditions on the cases the device has just been held to (a dictionary whose cases have
    not run in this session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _SEEN:
            _run_dictionary(device, spec)
    check_conditions([c for spec in DICTIONARIES for c in _SEEN[spec[0]]])
