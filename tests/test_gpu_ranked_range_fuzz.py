"""Differential fuzzing of the two docID-range ranked entries on the GPU: a few hundred seeded small indexes over random
dictionary files (tests/fuzz_streams.py: decoder-legal posting lists of one to a few blocks, wrapped freqs of 0 and freqs
near 2^32), each with a seeded query mix, a range per query — empty, inverted, one docID, on and beside the block maxima, up
to past the whole space — norm_lens of one class and a k of tests/query_fuzz_draws.py, under a seeded setting of the query
options, against the model (tests/ranked_range.py) and the blocks in range of the host block table."""
import numpy as np
import pytest

import fuzz_streams as F
import ranked
import ranked_range as RR
from query_fuzz_draws import CHOICES, KS, NORM_LENS, draw_norm_lens, query_mix

pytestmark = pytest.mark.gpu

CASES_PER_DICTIONARY = 40
# (seed, kind, docs dictionary shape, freqs dictionary shape): small dictionaries, two per kind
DICTIONARIES = [
    (31000, F.SINGLE, dict(m_entries=8, value_profile="tiny", size_profile="pow2"), dict(m_entries=9, value_profile="wide", size_profile="pow2")),
    (31001, F.SINGLE, dict(m_entries=300, value_profile="byte_edge", size_profile="any"), dict(m_entries=700, value_profile="tiny", size_profile="short")),
    (32000, F.RECT, dict(m_entries=256, value_profile="zeros", size_profile="sixteen"), dict(m_entries=257, value_profile="zeros", size_profile="pow2")),
    (32001, F.RECT, dict(m_entries=300, value_profile="byte_edge", size_profile="any"), dict(m_entries=3000, value_profile="mixed", size_profile="any")),
    (33000, F.MULTI, dict(m_entries=8, value_profile="tiny", size_profile="pow2"), dict(m_entries=700, value_profile="tiny", size_profile="short")),
    (33001, F.MULTI, dict(m_entries=300, value_profile="byte_edge", size_profile="any", context_entries=[300, 7, 300, 7, 30, 40]),
     dict(m_entries=9, value_profile="wide", size_profile="pow2")),
]


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


def draw_ranges(r, n, maxima, num_docs):
    """A range per query: anywhere, or with an end on, one below or one above a block maximum of the index"""
    out = []
    for _ in range(n):
        u = r.random()
        if u < 0.08:
            lo = int(r.integers(0, num_docs + 2))
            out.append((lo, lo - int(r.integers(0, 3)) if lo >= 2 else 0))  # empty or inverted
        elif u < 0.16:
            out.append((0, 0xFFFFFFFF) if r.random() < 0.5 else (0, num_docs))
        elif u < 0.5:
            a, b = (int(m) + int(r.integers(-1, 3)) for m in r.choice(maxima, 2))
            out.append((max(0, min(a, b)), max(a, b, 1)))
        else:
            width = int(np.exp(r.uniform(0.0, np.log(2.0 * num_docs))))
            lo = int(r.integers(0, num_docs))
            out.append((lo, min(lo + max(1, width), 0xFFFFFFFF)))
    return out


def run_range_case(device, dd, fd, Dd, Df, seed):
    r = np.random.default_rng(seed)
    X = F.make_index(r, Dd, Df, int(r.integers(6, 10)), max_n=900, value_cap=1 << 10)
    setting = {k: int(r.choice(v)) for k, v in CHOICES.items()}
    for k, v in setting.items():
        device.set_option(k, v)
    qs = query_mix(r, np.diff(X.bounds))[:20] + [[]]
    num_docs = int(X.docids.max()) + 1
    nl = draw_norm_lens(r, num_docs, NORM_LENS[int(r.integers(0, len(NORM_LENS)))])
    k = int(r.choice(KS))
    qi, wand = device.QueryIndex(dd, X.index, X.offsets), device.WandData(nl)
    ranges = draw_ranges(r, len(qs), qi.blocks["max"], num_docs)
    lists = ranked.BuilderLists(X.docids, X.freqs, X.bounds)
    lens = np.diff(X.bounds)
    matched = 0
    for entry, fn in (("or", qi.ranked_or_range_queries), ("and", qi.ranked_and_range_queries)):
        got = fn(fd, wand, qs, ranges, k=k, with_stats=True)
        want = [RR.top_in_range(RR.every_match(lists, q, nl, num_docs, entry == "and"), lo, hi, k) for q, (lo, hi) in zip(qs, ranges)]
        what = (seed, entry, k, setting)
        assert got[0].tolist() == [w[0] for w in want] and got[3].tolist() == [w[3] for w in want], what
        assert np.array_equal(got[1].view(np.uint32), np.stack([w[1] for w in want]).view(np.uint32)), what  # bit-equal scores
        assert np.array_equal(got[2], np.stack([w[2] for w in want])), what
        blocks = 0
        for q, (lo, hi) in zip(qs, ranges):
            terms = sorted(set(int(t) for t in q))
            if entry == "and" and terms:
                terms = [min(terms, key=lambda t: (int(lens[t]), t))]
            blocks += sum(RR.n_blocks_in_range(qi.blocks, t, lo, hi) for t in terms)
        assert got[4] == blocks, what
        i = int(r.integers(0, len(qs)))  # one query per call
        one = fn(fd, wand, [qs[i]], [ranges[i]], k=k, with_stats=True)
        assert _same_row(one, got, i), what
        matched += int(got[3].sum())
    qi.close()
    wand.close()
    device.reset_options()
    return matched


@pytest.mark.parametrize("spec", DICTIONARIES, ids=lambda s: f"seed{s[0]}")
def test_range_cases(device, spec):
    seed, kind, ds, fs = spec
    r = np.random.default_rng(seed)
    Dd, Df = F.make_dictionary(r, kind, **ds), F.make_dictionary(r, kind, **fs)
    dd, fd = device.Dictionary(Dd.kind, Dd.file), device.Dictionary(Df.kind, Df.file)
    matched = sum(run_range_case(device, dd, fd, Dd, Df, 100 * seed + i) for i in range(CASES_PER_DICTIONARY))
    assert matched > 500 * CASES_PER_DICTIONARY // 40, "the cases match something"
