"""Differential fuzzing of the two document-filter ranked entries on the GPU: a few hundred seeded small indexes over random
dictionary files (tests/fuzz_streams.py: decoder-legal posting lists of one to a few blocks, wrapped freqs of 0 and freqs
near 2^32), each with a seeded query mix, ONE filter of a random kind for the case (tests/doc_filter.py's fuzz_filter: runs
around postings, a few documents, an interval, one term's documents, their complement, densities 1/2 and 1/64, all, none,
with a num_docs below, at or above the index's), norm_lens of one class and a k of tests/query_fuzz_draws.py, under a seeded
setting of the query options, against the model (tests/doc_filter.py) and the live blocks of the host block table.

Two conditions on the committed seeds, asserted here on what the device returns — of EITHER entry — and replayed from the
model alone by tests/test_doc_filter_cpu.py (check_shares): of the (case, query) pairs, at least half match something, and at
least a quarter decode strictly fewer blocks than the unfiltered call. The draws are made to meet them (draw_filter_case: most
of a case's queries are ones whose lists share a document; the clustered filters lie around such documents). The device
reports blocks_decoded per call: the test holds the batch's total to the sum of the model's per-query counts, one query per
case alone to its own count, and takes the shares from the per-query counts."""
import collections
import functools

import numpy as np
import pytest

import doc_filter as DF
import fuzz_streams as F
import ranked
from query_fuzz_draws import CHOICES, KS, NORM_LENS, draw_norm_lens, query_mix

pytestmark = pytest.mark.gpu

CASES_PER_DICTIONARY = 40
# (seed, kind, docs dictionary shape, freqs dictionary shape): small dictionaries, two per kind
DICTIONARIES = [
    (41000, F.SINGLE, dict(m_entries=8, value_profile="tiny", size_profile="pow2"), dict(m_entries=9, value_profile="wide", size_profile="pow2")),
    (41001, F.SINGLE, dict(m_entries=300, value_profile="byte_edge", size_profile="any"), dict(m_entries=700, value_profile="tiny", size_profile="short")),
    (42000, F.RECT, dict(m_entries=256, value_profile="zeros", size_profile="sixteen"), dict(m_entries=257, value_profile="zeros", size_profile="pow2")),
    (42001, F.RECT, dict(m_entries=300, value_profile="byte_edge", size_profile="any"), dict(m_entries=3000, value_profile="mixed", size_profile="any")),
    (43000, F.MULTI, dict(m_entries=8, value_profile="tiny", size_profile="pow2"), dict(m_entries=700, value_profile="tiny", size_profile="short")),
    (43001, F.MULTI, dict(m_entries=300, value_profile="byte_edge", size_profile="any", context_entries=[300, 7, 300, 7, 30, 40]),
     dict(m_entries=9, value_profile="wide", size_profile="pow2")),
]
ENTRIES = (("or", False), ("and", True))

FilterCase = collections.namedtuple("FilterCase", "seed X setting qs num_docs nl k kind mask pick")


QUERIES_PER_CASE, INTERSECTING_PER_CASE = 20, 17


def intersection_of(X, q):
    """the documents every list of q holds (from the builder's input: no codec, no model)"""
    own = [X.docids[int(X.bounds[t]):int(X.bounds[t + 1])] for t in sorted(set(int(t) for t in q))]
    return functools.reduce(lambda a, b: np.intersect1d(a, b, assume_unique=True), own)


def draw_filter_case(Dd, Df, seed):
    """Everything a case draws, in this order from one generator: the index, the options, the queries, norm_lens, k, the
    filter, and the query that is also asked alone. The queries are query_mix's without the empty ones, in its order: the
    first INTERSECTING_PER_CASE whose lists share a document, then others up to QUERIES_PER_CASE — the plain mix's
    intersection is empty for half of its queries, whatever the filter, and the conditions below are asked of the AND
    entry too. The clustered filters are drawn around documents of those intersections."""
    r = np.random.default_rng(seed)
    X = F.make_index(r, Dd, Df, int(r.integers(6, 10)), max_n=900, value_cap=1 << 10)
    setting = {k: int(r.choice(v)) for k, v in CHOICES.items()}
    mix = [q for q in query_mix(r, np.diff(X.bounds)) if len(q)]
    shared = [intersection_of(X, q) for q in mix]
    first = [i for i in range(len(mix)) if shared[i].size][:INTERSECTING_PER_CASE]
    chosen = sorted(first + [i for i in range(len(mix)) if i not in first][:QUERIES_PER_CASE - len(first)])
    qs = [mix[i] for i in chosen]
    num_docs = int(X.docids.max()) + 1
    nl = draw_norm_lens(r, num_docs, NORM_LENS[int(r.integers(0, len(NORM_LENS)))])
    k = int(r.choice(KS))
    kind, mask = DF.fuzz_filter(r, X.docids, X.bounds, np.concatenate([shared[i] for i in chosen]))
    return FilterCase(seed, X, setting, qs, num_docs, nl, k, kind, mask, int(r.integers(0, len(qs))))


def model_of(case, table):
    """-> {entry: (the model's per-query (count, scores, docids, matches), per-query live blocks, per-query blocks unfiltered,
    per-query matches unfiltered)}"""
    lists = ranked.BuilderLists(case.X.docids, case.X.freqs, case.X.bounds)
    lens = np.diff(case.X.bounds)
    live = DF.live_blocks(table, case.mask)
    out = {}
    for entry, conjunctive in ENTRIES:
        every = [DF.every_match(lists, q, case.nl, case.num_docs, conjunctive) for q in case.qs]
        want = [DF.top_in_filter(e, case.mask, case.k) for e in every]
        out[entry] = (want, [DF.planned_blocks(table, live, lens, q, conjunctive) for q in case.qs],
                      [DF.planned_blocks(table, None, lens, q, conjunctive) for q in case.qs], [int(e[1].size) for e in every])
    return out


def shares_of(matches, blocks, unfiltered_blocks, unfiltered_matches):
    """-> (pairs, the pairs that match something, those that decode strictly fewer blocks than the unfiltered call, those
    that match something unfiltered)"""
    return (len(blocks), sum(int(m) > 0 for m in matches), sum(b < u for b, u in zip(blocks, unfiltered_blocks)),
            sum(int(m) > 0 for m in unfiltered_matches))


def model_shares(case, table):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    m = model_of(case, table)
    return [shares_of([w[3] for w in m[e][0]], m[e][1], m[e][2], m[e][3]) for e, _ in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the two conditions of this file's docstring, of either entry"""
    for (entry, _), (pairs, matched, skipping, matchable) in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "pairs", pairs, "matched", matched, "skipping", skipping, "match unfiltered", matchable)
        assert pairs >= QUERIES_PER_CASE * CASES_PER_DICTIONARY * len(DICTIONARIES)
        assert 2 * matched >= pairs, (entry, matched, pairs)
        assert 4 * skipping >= pairs, (entry, skipping, pairs)


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


def _same_row(one, got, i):
    return all(np.asarray(one[j][0]).tobytes() == np.asarray(got[j][i]).tobytes() for j in range(4))


def run_filter_case(device, dd, fd, Dd, Df, seed):
    case = draw_filter_case(Dd, Df, seed)
    for k, v in case.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, case.X.index, case.X.offsets), device.WandData(case.nl)
    model = model_of(case, qi.blocks)
    f = qi.doc_filter(case.mask)
    info = f.info
    live = DF.live_blocks(qi.blocks, case.mask)
    what = (seed, case.kind, case.k, case.setting)
    assert (info.num_docs, info.n_set, info.n_blocks, info.live_blocks) == (case.mask.size, int(case.mask.sum()), len(qi.blocks), int(live.sum())), what
    shares = []
    for (entry, _), fn in zip(ENTRIES, (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
        want, blocks, unfiltered, unfiltered_matches = model[entry]
        got = fn(fd, wand, case.qs, f, k=case.k, with_stats=True)
        assert got[0].tolist() == [w[0] for w in want] and got[3].tolist() == [w[3] for w in want], what + (entry,)
        assert np.array_equal(got[1].view(np.uint32), np.stack([w[1] for w in want]).view(np.uint32)), what + (entry,)  # bit-equal scores
        assert np.array_equal(got[2], np.stack([w[2] for w in want])), what + (entry,)
        assert got[4] == sum(blocks), what + (entry,)
        i = case.pick  # one query per call: its own row and its own blocks
        one = fn(fd, wand, [case.qs[i]], f, k=case.k, with_stats=True)
        assert _same_row(one, got, i) and one[4] == blocks[i], what + (entry,)
        shares.append(shares_of(got[3], blocks, unfiltered, unfiltered_matches))
    f.close()
    qi.close()
    wand.close()
    device.reset_options()
    return shares


_TOTALS = {}  # {dictionary seed: shares_of summed over its cases, per entry}


def _run_dictionary(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = F.make_dictionary(r, kind, **ds), F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    _TOTALS[seed] = np.sum([run_filter_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_filter_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_cases_match_and_skip_enough(device):
    """Over all the cases above: check_shares on what the device returned (a dictionary whose cases have not run in this
    session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    check_shares(np.sum([_TOTALS[spec[0]] for spec in DICTIONARIES], axis=0))
