"""Differential fuzzing of the two collapsed ranked entries on the GPU: 240 seeded small indexes over the random dictionary
files of tests/test_gpu_doc_filter_fuzz.py, drawn as tests/test_gpu_facets_fuzz.py draws its cases (decoder-legal posting
lists of one to a few blocks, a seeded query mix, norm_lens, k, option settings and a filter), each with ONE group map of a
random kind (tests/collapse.py's fuzz_map: clustered, striped, random, one group, none, every other document NONE; n_groups in
1 .. 600, so both forms of collapse_best_kernel; a map that ends below, at or above the index's largest docID). The case's
filter is used in half of the cases. Every output is held to the model (tests/collapse.py), bit for bit, and matches,
blocks_decoded and the rows to the faceted entry's on the same arguments.

Two conditions on the committed seeds keep the test from passing vacuously. They are asserted here on what the device returns
— of EITHER entry — and replayed from the model alone by tests/test_collapse_cpu.py (check_shares): of the (case, query)
pairs, at least half have collapsed < matches (collapsing removed something), and at least half have collapsed >= 2 (the
selection still has something to order). The draws are made to meet them (draw_collapse_case: most of a case's queries are
ones whose lists share many documents; tests/collapse.py's fuzz_map: few groups and clustered kinds weigh most).
Reached by the committed seeds, from the model (4800 pairs an entry) — OR: 4167 with collapsed < matches, 3612 with
collapsed >= 2; AND: 3075 with collapsed < matches, 2528 with collapsed >= 2."""
import collections

import numpy as np
import pytest

import collapse as CO
import doc_filter as DF
import ranked
import test_gpu_doc_filter_fuzz as Z

pytestmark = pytest.mark.gpu

DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Z.DICTIONARIES, Z.CASES_PER_DICTIONARY, Z.ENTRIES

CollapseCase = collections.namedtuple("CollapseCase", "base map_kind n_groups group_of mask")

SHARED = 12  # a query whose lists share at least this many documents can lose some to collapsing and still keep two


def draw_collapse_case(Dd, Df, seed):
    """Everything a case draws, in this order from one generator: the filter fuzz's draws (Z.draw_filter_case: the index, the
    options, the queries, norm_lens, k, the filter, the query that is also asked alone) with one difference — of the query
    mix, the first Z.INTERSECTING_PER_CASE queries whose lists share at least SHARED documents are taken, not the first that
    share one: a conjunctive query with a match or two has nothing to collapse — then the map, and whether the case's filter
    is used (mask None: no filter)."""
    r = np.random.default_rng(seed)
    X = Z.F.make_index(r, Dd, Df, int(r.integers(6, 10)), max_n=900, value_cap=1 << 10)
    setting = {k: int(r.choice(v)) for k, v in Z.CHOICES.items()}
    mix = [q for q in Z.query_mix(r, np.diff(X.bounds)) if len(q)]
    shared = [Z.intersection_of(X, q) for q in mix]
    first = [i for i in range(len(mix)) if shared[i].size >= SHARED][:Z.INTERSECTING_PER_CASE]
    chosen = sorted(first + [i for i in range(len(mix)) if i not in first][:Z.QUERIES_PER_CASE - len(first)])
    qs = [mix[i] for i in chosen]
    num_docs = int(X.docids.max()) + 1
    nl = Z.draw_norm_lens(r, num_docs, Z.NORM_LENS[int(r.integers(0, len(Z.NORM_LENS)))])
    k = int(r.choice(Z.KS))
    kind, mask = DF.fuzz_filter(r, X.docids, X.bounds, np.concatenate([shared[i] for i in chosen]))
    base = Z.FilterCase(seed, X, setting, qs, num_docs, nl, k, kind, mask, int(r.integers(0, len(qs))))
    map_kind, n_groups, group_of = CO.fuzz_map(r, num_docs)
    return CollapseCase(base, map_kind, n_groups, group_of, mask if r.random() < 0.5 else None)


def model_of(case):
    """-> {entry: per query tests/collapse.py's collapse tuple}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    return {entry: [CO.collapse(CO.every_match(lists, q, b.nl, b.num_docs, conjunctive), case.mask, case.group_of, case.n_groups, b.k)
                    for q in b.qs] for entry, conjunctive in ENTRIES}


def shares_of(matches, collapsed):
    """-> (pairs, the pairs with collapsed < matches, the pairs with collapsed >= 2)"""
    return (len(matches), sum(int(c) < int(m) for m, c in zip(matches, collapsed)), sum(int(c) >= 2 for c in collapsed))


def model_shares(case):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    m = model_of(case)
    return [shares_of([w[3] for w in m[e]], [w[4] for w in m[e]]) for e, _ in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the two conditions of this file's docstring, of either entry"""
    for (entry, _), (pairs, less, two) in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "pairs", pairs, "collapsed < matches", less, "collapsed >= 2", two)
        assert pairs >= Z.QUERIES_PER_CASE * CASES_PER_DICTIONARY * len(DICTIONARIES)
        assert 2 * less >= pairs, (entry, less, pairs)
        assert 2 * two >= pairs, (entry, two, pairs)


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


def run_collapse_case(device, dd, fd, Dd, Df, seed):
    case = draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    model = model_of(case)
    facets = device.DocFacets(0, case.group_of, case.n_groups)
    what = (seed, case.map_kind, case.n_groups, len(case.group_of), case.mask is not None, b.k, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    shares = []
    for (entry, _), fn, plain in zip(ENTRIES, (qi.ranked_or_collapsed_queries, qi.ranked_and_collapsed_queries),
                                     (qi.ranked_or_faceted_queries, qi.ranked_and_faceted_queries)):
        want = CO.stacked(model[entry], b.k, case.n_groups)
        got = fn(fd, wand, b.qs, facets, filter=f, k=b.k, with_stats=True, with_rows=True)
        _bit_equal(got[:4] + got[5:], want, what + (entry,))
        same = plain(fd, wand, b.qs, facets, filter=f, k=b.k, with_stats=True)
        _bit_equal((got[3], got[8]), (same[3], same[5]), what + (entry,))
        assert got[4] == same[4], what + (entry,)
        i = b.pick  # one query per call, without the rows: its own answer
        one = fn(fd, wand, [b.qs[i]], facets, filter=f, k=b.k)
        _bit_equal([x[0] for x in one], [want[j][i] for j in (0, 1, 2, 4, 5, 6)], what + (entry,))
        shares.append(shares_of(got[3], got[5]))
    if f is not None:
        f.close()
    facets.close()
    qi.close()
    wand.close()
    device.reset_options()
    return shares


_TOTALS = {}  # {dictionary seed: shares_of summed over its cases, per entry}


def _run_dictionary(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    _TOTALS[seed] = np.sum([run_collapse_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_collapse_cases(device, spec):
    _run_dictionary(device, spec)


def test_collapsing_removes_and_keeps_enough(device):
    """Over all the cases above: check_shares on what the device returned (a dictionary whose cases have not run in this
    session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    check_shares(np.sum([_TOTALS[spec[0]] for spec in DICTIONARIES], axis=0))
