"""Differential fuzzing of the four paged ranked entries on the GPU, over the 240 cases of tests/test_gpu_collapse_fuzz.py
(draw_collapse_case, imported: seeded small indexes, a query mix, norm_lens, k, option settings, a filter used in half of the
cases and one group map). Per (case, entry, query) one cursor is drawn from a generator of its own,
np.random.default_rng([case seed, 0x5AF7]) (tests/paging.py's draw_cursors), so the base draws do not shift: with probability
0.7 a uniformly drawn match of the query under the case's mask, 0.1 a match's score with a random docID in [0, num_docs + 2),
0.1 from the start, 0.1 a random score in (0, 1.1 x the best score) with a random docID; a query without a match gets no draw.
The paged entries are held to the model (tests/paging.py), bit for bit; the collapsed paged entries to the model on the case's
map, under the same cursors; a from-the-start call to the filtered entry.

Two conditions on the committed seeds keep the test from passing vacuously. They are asserted here on what the device returns
— of EITHER plain entry — and replayed from the model alone by tests/test_paging_cpu.py (check_shares): of the (case, query)
pairs, in at least half the cursor splits the matches (0 < skipped < matches), and in at least one in ten a match with the
cursor's score lies on each side of the cut.
Reached by the committed seeds and these weights, from the model (4800 pairs an entry) — OR: 3739 splits, 847 ties;
AND: 2741 splits, 568 ties."""
import numpy as np
import pytest

import paging as PG
import ranked
import test_gpu_collapse_fuzz as Y

pytestmark = pytest.mark.gpu

Z = Y.Z
DICTIONARIES, CASES_PER_DICTIONARY, ENTRIES = Y.DICTIONARIES, Y.CASES_PER_DICTIONARY, Y.ENTRIES


def every_of(case):
    """-> {entry: per query every match of the unfiltered model}"""
    b = case.base
    lists = ranked.BuilderLists(b.X.docids, b.X.freqs, b.X.bounds)
    return {entry: [PG.CO.every_match(lists, q, b.nl, b.num_docs, conjunctive) for q in b.qs] for entry, conjunctive in ENTRIES}


def cursors_of(case, every):
    return PG.draw_cursors(case.base.seed, every, case.mask, case.base.num_docs)


def shares_of(every, mask, cursors):
    """one entry's queries -> (pairs, the pairs the cursor splits, the pairs with the cursor's score on each side of the cut)"""
    st = [PG.split_and_tie(m, mask, c) for m, c in zip(every, cursors)]
    return len(st), sum(s for s, _ in st), sum(t for _, t in st)


def model_shares(case):
    """-> the case's shares_of per entry [or, and], from the model alone"""
    every = every_of(case)
    cursors = cursors_of(case, every)
    return [shares_of(every[e], case.mask, cursors[e]) for e, _ in ENTRIES]


def check_shares(per_entry):
    """per_entry: shares_of summed over the cases, [or, and] — the two conditions of this file's docstring, of either entry"""
    for (entry, _), (pairs, splits, ties) in zip(ENTRIES, (tuple(int(x) for x in e) for e in per_entry)):
        print(entry, "pairs", pairs, "splits", splits, "ties", ties)
        assert pairs >= Z.QUERIES_PER_CASE * CASES_PER_DICTIONARY * len(DICTIONARIES)
        assert 2 * splits >= pairs, (entry, splits, pairs)
        assert 10 * ties >= pairs, (entry, ties, pairs)


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


def run_paging_case(device, dd, fd, Dd, Df, seed):
    case = Y.draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    cursors = cursors_of(case, every)
    facets = device.DocFacets(0, case.group_of, case.n_groups)
    what = (seed, case.map_kind, case.n_groups, case.mask is not None, b.k, b.setting)
    f = qi.doc_filter(case.mask) if case.mask is not None else None
    shares = []
    for (entry, _), paged, collapsed_paged, filtered in zip(
            ENTRIES, (qi.ranked_or_paged_queries, qi.ranked_and_paged_queries),
            (qi.ranked_or_collapsed_paged_queries, qi.ranked_and_collapsed_paged_queries),
            (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
        after = cursors[entry]
        want = PG.stacked([PG.page_after(m, case.mask, c, b.k) for m, c in zip(every[entry], after)], b.k)
        got = paged(fd, wand, b.qs, after=after, filter=f, k=b.k, with_stats=True)
        _bit_equal(got[:4] + got[5:], want, what + (entry,))
        same = filtered(fd, wand, b.qs, f, k=b.k, with_stats=True)
        _bit_equal((got[3],), (same[3],), what + (entry,))
        assert got[4] == same[4], what + (entry,)
        start = paged(fd, wand, b.qs, after=None, filter=f, k=b.k, with_stats=True)  # from the start: the filtered entry's answer
        _bit_equal(start[:4], same[:4], what + (entry, "from the start"))
        assert start[4] == same[4] and not start[5].any(), what + (entry,)
        i = b.pick  # one query per call: its own answer
        one = paged(fd, wand, [b.qs[i]], after=[after[i]], filter=f, k=b.k)
        _bit_equal([x[0] for x in one], [want[j][i] for j in (0, 1, 2, 4)], what + (entry,))
        want_c = PG.collapsed_stacked([PG.collapsed_page_after(m, case.mask, case.group_of, case.n_groups, c, b.k)
                                       for m, c in zip(every[entry], after)], b.k, case.n_groups)
        got_c = collapsed_paged(fd, wand, b.qs, facets, after=after, filter=f, k=b.k, with_stats=True, with_rows=True)
        _bit_equal(got_c[:4] + got_c[5:], want_c, what + (entry, "collapsed"))
        assert got_c[4] == same[4], what + (entry,)
        # the conditions: the split share is counted from the device's skipped and matches. The tie share is counted from the
        # MODEL's matches (a page does not return what lies in front of the cut), which the device's outputs have just been
        # held to bit for bit; of the device it is required besides that the page begins with the cursor's score
        st = [PG.split_and_tie(m, case.mask, c) for m, c in zip(every[entry], after)]
        assert [bool(0 < s < m) for s, m in zip(got[5], got[3])] == [s for s, _ in st], what + (entry,)
        for q, (_, tie) in enumerate(st):
            assert not tie or got[1][q, 0].tobytes() == np.float32(after[q][0]).tobytes(), what + (entry, q)
        shares.append((len(b.qs), sum(bool(0 < s < m) for s, m in zip(got[5], got[3])), sum(t for _, t in st)))
    if f is not None:
        f.close()
    facets.close()
    qi.close()
    wand.close()
    device.reset_options()
    return shares


_TOTALS = {}  # {dictionary seed: the shares summed over its cases, per entry}


def _run_dictionary(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    _TOTALS[seed] = np.sum([run_paging_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY)], axis=0)


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_paging_cases(device, spec):
    _run_dictionary(device, spec)


def test_the_cursors_split_and_tie_often_enough(device):
    """Over all the cases above: check_shares on what the device returned (a dictionary whose cases have not run in this
    session — this test asked for alone — runs here)."""
    for spec in DICTIONARIES:
        if spec[0] not in _TOTALS:
            _run_dictionary(device, spec)
    check_shares(np.sum([_TOTALS[spec[0]] for spec in DICTIONARIES], axis=0))
