"""Differential fuzzing of the two faceted ranked entries on the GPU: 240 seeded small indexes over the random dictionary
files of tests/test_gpu_doc_filter_fuzz.py, drawn as that file draws its cases (decoder-legal posting lists of one to a few
blocks, a seeded query mix, norm_lens, k, option settings and a filter), each with ONE group map of a random kind
(tests/facets.py's fuzz_map: clustered, striped, random, one group, none, every other document NONE; n_groups in 1 .. 600, so
both forms of the counting kernel; a map that ends below, at or above the index's largest docID). The case's filter is used in
half of the cases. The ranked outputs and blocks_decoded are held to the filtered entry's on the same arguments, bit for bit,
and to the model; the rows to numpy.bincount over the model's matches (tests/facets.py).

Two conditions on the committed seeds keep the test from passing vacuously. They are asserted here on what the device returns
— of EITHER entry — and replayed from the model alone by tests/test_facets_cpu.py (check_shares): of the (case, query) pairs,
at least half match something, and at least half have their matches in at least two groups. The draws are made to meet them
(draw_facet_case: most of a case's queries are ones whose lists share several documents).
Reached by the committed seeds, from the model (4800 pairs an entry) — OR: 4577 match, 3689 in two groups or more; AND: 3656
match, 2559 in two groups or more."""
import collections

import numpy as np
import pytest

import doc_filter as DF
import facets as FA
import ranked
import test_gpu_doc_filter_fuzz as Z

pytestmark = pytest.mark.gpu

DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Z.DICTIONARIES, Z.CASES_PER_DICTIONARY, Z.ENTRIES

FacetCase = collections.namedtuple("FacetCase", "base map_kind n_groups group_of mask")

SPREADABLE = 4  # a query whose lists share at least this many documents can have its AND matches in several groups


def draw_facet_case(Dd, Df, seed):
    """Everything a case draws, in this order from one generator: the filter fuzz's draws (Z.draw_filter_case: the index, the
    options, the queries, norm_lens, k, the filter, the query that is also asked alone) with one difference — of the query
    mix, the first Z.INTERSECTING_PER_CASE queries whose lists share at least SPREADABLE documents are taken, not the first
    that share one: a conjunctive query with a single match cannot spread over two groups, whatever the map — then the map,
    and whether the case's filter is used (mask None: no filter)."""
    r = np.random.default_rng(seed)
    X = Z.F.make_index(r, Dd, Df, int(r.integers(6, 10)), max_n=900, value_cap=1 << 10)
    setting = {k: int(r.choice(v)) for k, v in Z.CHOICES.items()}
    mix = [q for q in Z.query_mix(r, np.diff(X.bounds)) if len(q)]
    shared = [Z.intersection_of(X, q) for q in mix]
    first = [i for i in range(len(mix)) if shared[i].size >= SPREADABLE][:Z.INTERSECTING_PER_CASE]
    chosen = sorted(first + [i for i in range(len(mix)) if i not in first][:Z.QUERIES_PER_CASE - len(first)])
    qs = [mix[i] for i in chosen]
    num_docs = int(X.docids.max()) + 1
    nl = Z.draw_norm_lens(r, num_docs, Z.NORM_LENS[int(r.integers(0, len(Z.NORM_LENS)))])
    k = int(r.choice(Z.KS))
    kind, mask = DF.fuzz_filter(r, X.docids, X.bounds, np.concatenate([shared[i] for i in chosen]))
    base = Z.FilterCase(seed, X, setting, qs, num_docs, nl, k, kind, mask, int(r.integers(0, len(qs))))
    map_kind, n_groups, group_of = FA.fuzz_map(r, num_docs)
    return FacetCase(base, map_kind, n_groups, group_of, mask if r.random() < 0.5 else None)


def model_of(case):
    """-> {entry: per query (the model's (count, scores, docids, matches), its row, its matches in no group)}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    mask = case.mask if case.mask is not None else np.ones(b.num_docs, dtype=bool)  # (no filter: every document of the index)
    out = {}
    for entry, conjunctive in ENTRIES:
        per_query = []
        for q in b.qs:
            every = DF.every_match(lists, q, b.nl, b.num_docs, conjunctive)
            per_query.append((DF.top_in_filter(every, mask, b.k),) + FA.row_of(case.group_of, case.n_groups, FA.matches_in(every, case.mask)))
        out[entry] = per_query
    return out


def shares_of(matches, rows):
    """-> (pairs, the pairs that match something, the pairs whose matches fall in at least two groups)"""
    return (len(rows), sum(int(m) > 0 for m in matches), sum(int(np.count_nonzero(row)) >= 2 for row in rows))


def model_shares(case):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    m = model_of(case)
    return [shares_of([w[0][3] for w in m[e]], [w[1] for w in m[e]]) for e, _ in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the two conditions of this file's docstring, of either entry"""
    for (entry, _), (pairs, matched, spread) in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "pairs", pairs, "matched", matched, "in two groups or more", spread)
        assert pairs >= Z.QUERIES_PER_CASE * CASES_PER_DICTIONARY * len(DICTIONARIES)
        assert 2 * matched >= pairs, (entry, matched, pairs)
        assert 2 * spread >= pairs, (entry, spread, pairs)


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


def run_facet_case(device, dd, fd, Dd, Df, seed):
    case = draw_facet_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    model = model_of(case)
    facets = device.DocFacets(0, case.group_of, case.n_groups)
    sizes, n_grouped = FA.sizes_of(case.group_of, case.n_groups)
    what = (seed, case.map_kind, case.n_groups, len(case.group_of), case.mask is not None, b.k, b.setting)
    assert (facets.num_docs, facets.n_groups, facets.n_grouped) == (len(case.group_of), case.n_groups, n_grouped), what
    assert np.array_equal(facets.group_sizes, sizes), what
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    shares = []
    for (entry, _), fn, plain in zip(ENTRIES, (qi.ranked_or_faceted_queries, qi.ranked_and_faceted_queries),
                                     (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
        want = model[entry]
        got = fn(fd, wand, b.qs, facets, filter=f, k=b.k, with_stats=True)
        same = plain(fd, wand, b.qs, f, k=b.k, with_stats=True)
        _bit_equal(got[:4], same[:4], what + (entry,))
        assert got[4] == same[4], what + (entry,)
        assert got[0].tolist() == [w[0][0] for w in want] and got[3].tolist() == [w[0][3] for w in want], what + (entry,)
        assert np.array_equal(got[1].view(np.uint32), np.stack([w[0][1] for w in want]).view(np.uint32)), what + (entry,)
        assert np.array_equal(got[2], np.stack([w[0][2] for w in want])), what + (entry,)
        rows = got[5]
        assert rows.dtype == np.uint32 and rows.shape == (len(b.qs), case.n_groups)
        assert np.array_equal(rows, np.stack([w[1] for w in want])), what + (entry,)
        assert (rows.sum(axis=1, dtype=np.int64) + np.array([w[2] for w in want]) == got[3].astype(np.int64)).all(), what + (entry,)
        i = b.pick  # one query per call: its own row
        one = fn(fd, wand, [b.qs[i]], facets, filter=f, k=b.k, with_stats=True)
        assert np.array_equal(one[5][0], rows[i]) and one[3][0] == got[3][i], what + (entry,)
        shares.append(shares_of(got[3], rows))
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
    _TOTALS[seed] = np.sum([run_facet_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_facet_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_cases_match_and_spread_enough(device):
    """Over all the cases above: check_shares on what the device returned (a dictionary whose cases have not run in this
    session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    check_shares(np.sum([_TOTALS[spec[0]] for spec in DICTIONARIES], axis=0))
