"""Differential fuzzing of the two top-values ranked entries on the GPU, over a handful of the cases of
tests/test_gpu_percentiles_fuzz.py (draw_collapse_case: seeded small indexes, a query mix, norm_lens, k, option settings, a
filter): the first CASES of every dictionary. Per case the column and n_top come from a generator of the case's own,
np.random.default_rng([case seed, 0x70B5]) (tests/top_values.py's draw_case): a column of few values, of many or of values that
are all distinct, in a quarter of the cases shorter than the index's docID space, and n_top 0, small, around the selection's run
sizes or 1024. Both entries run without a filter and under the case's filter, and are held to the model (tests/top_values.py)
count for count and value for value; their ranked outputs, matches and blocks_decoded to the filtered entry's, bit for bit; and
one query to the model asked alone. Every drawn case is checked; none is skipped.

What the handful covers is a property of the draws, settled from the model alone by tests/test_top_values_cpu.py
(test_the_fuzz_cases_cover_their_ground): every kind of column, a short column, n_top 0 and n_top >= 256, a query with more
distinct values than n_top, and a query with more than 256 valued matches, so that pages meet in a table."""
import numpy as np
import pytest

import test_gpu_collapse_fuzz as Y
import test_gpu_value_stats_fuzz as S
import top_values as TV

pytestmark = pytest.mark.gpu

Z = Y.Z
DICTIONARIES, ENTRIES = Y.DICTIONARIES, Y.ENTRIES
CASES = 5  # per dictionary

every_of = S.every_of
_bit_equal = S._bit_equal


def case_seeds(spec):
    return [100 * spec[0] + i for i in range(CASES)]


def draws_of(case):
    """-> (the column's kind, values, n_top)"""
    return TV.draw_case(case.base.seed, case.base.num_docs)


def coverage_of(case):
    """one case, from the model alone -> (kind, a short column, n_top, some query with more distinct values than n_top, some
    query with more than 256 valued matches)"""
    kind, values, n_top = draws_of(case)
    every = every_of(case)
    models = [TV.top_values(m, mask, values, n_top) for e, _ in ENTRIES for mask in (None, case.base.mask) for m in every[e]]
    return kind, len(values) < case.base.num_docs, n_top, any(o[1] > n_top > 0 for o in models), any(o[0] > 256 for o in models)


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


def run_top_values_case(device, dd, fd, Dd, Df, seed):
    case = Y.draw_collapse_case(Dd, Df, seed)
    b = case.base
    for k, v in b.setting.items():
        device.set_option(k, v)
    qi, wand = device.QueryIndex(dd, b.X.index, b.X.offsets), device.WandData(b.nl)
    every = every_of(case)
    kind, values, n_top = draws_of(case)
    col = device.DocValues(0, values)
    f = qi.doc_filter(b.mask)
    for mask, filt in ((None, None), (b.mask, f)):
        what = (seed, kind, len(values), b.num_docs, n_top, mask is not None, b.k, b.setting)
        for (entry, _), call, filtered in zip(ENTRIES, (qi.ranked_or_top_values_queries, qi.ranked_and_top_values_queries),
                                              (qi.ranked_or_filtered_queries, qi.ranked_and_filtered_queries)):
            model = [TV.top_values(m, mask, values, n_top) for m in every[entry]]
            same = filtered(fd, wand, b.qs, filt, k=b.k, with_stats=True)
            got = call(fd, wand, b.qs, col, n_top, filter=filt, k=b.k)
            _bit_equal(got[:4], same[:4], what + (entry, "the ranked outputs"))
            assert got[4] == same[4], what + (entry,)
            _bit_equal(got[5:], TV.stacked(model, n_top), what + (entry,))
            i = b.pick  # one query per call: its own answer
            one = call(fd, wand, [b.qs[i]], col, n_top, filter=filt, k=b.k)
            _bit_equal(one[5:], TV.stacked([model[i]], n_top), what + (entry, "alone"))
    for h in (f, col, qi, wand):
        h.close()
    device.reset_options()


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_top_values_cases(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = Z.F.make_dictionary(r, kind, **ds), Z.F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    for case_seed in case_seeds(spec):
        run_top_values_case(device, dd, fd, Dd, Df, case_seed)
