"""The plain model of the device's n-gram statistics (tests/ngram_stats.py) against the oracle's restatement of the
reference (oracle/dint_oracle_stats.c) and against the host library's selection, and the named cases and fuzz draws of
tests/test_gpu_ngram_stats.py checked to be what they are said to be — all without a GPU. Everything is an integer or one
double comparison: no tolerance anywhere."""
import numpy as np
import pytest

import ngram_stats as NS
import oracle
from dint_amd import host

ALL = [NS.cases()[n] for n in NS.CASE_NAMES] + NS.draws()
KINDS = [host.RECTANGULAR, host.SINGLE_PACKED, host.MULTI_PACKED]
M32 = NS.M32


def test_the_models_entry_is_the_librarys():
    assert NS.NGRAM_DTYPE == host.NGRAM_DTYPE and NS.NGRAM_DTYPE.itemsize == 16
    k = host.constants()
    assert list(NS.WIDTHS) == k["target_sizes"] and k["num_selectors"] == 6 and sum(NS.BLOCK // w for w in NS.WIDTHS) == NS.NGRAMS_PER_CHUNK


def test_context_of_by_hand():
    for m, c in NS.CONTEXT_EDGES.items():
        assert NS.context_of(m) == c == oracle.selector_get(np.array([0, m], dtype=np.uint32)), m
    assert [NS.context_of(m) for m in (5, 100, 1000, 2**31, 2**32 - 3)] == [2, 3, 4, 5, 5]


@pytest.mark.parametrize("case", ALL, ids=lambda c: c.name)
def test_model_against_oracle(case):
    """counts, first positions, the selection and the total: the oracle meets an n-gram first at its smallest position (lists in
    order, one width after the other), so its `pos` is the model's first_pos"""
    st = oracle.Stats(case.multi, case.gaps)
    st.collect_lists(case.lens)
    want = {(c, st.ngram(e)): (int(e["freq"]), int(e["pos"])) for c in range(st.contexts) for e in st.entries(c)}
    assert case.counts == want
    assert case.total == st.total_integers == sum(case.lens)
    chosen = NS.select(case.entries, case.gaps, case.total, 65536)
    want_sel = [(c, int(e["len"]), int(e["freq"]), int(e["pos"])) for c in range(st.contexts) for e in st.select(c)[0]]
    assert NS.as_list(chosen) == want_sel
    # and the cut loses nothing the selection takes
    for top_k in {1, 8, getattr(case, "top_k", 3)}:
        back = NS.cut(case.entries, case.total, top_k)
        assert NS.as_list(NS.select(back, case.gaps, case.total, top_k)) == NS.as_list(NS.select(case.entries, case.gaps, case.total, top_k))


def test_filter_brackets_by_hand():
    """freq 1: a pair saves 80 / total, 4, 8 and 16 integers 176, 368 and 752 / total; 1e7 times that is the double 1e-07 itself,
    one ulp below 0.0001 / 1000"""
    assert 0.0001 / 1000 == 1.0000000000000001e-07 > 1e-7 and np.nextafter(1e-7, 1.0) == 0.0001 / 1000
    for length, m in ((2, 80), (4, 176), (8, 368), (16, 752)):
        assert 1 * (48.0 * length - 16.0) / float(m * 10**7) == 1e-7
        assert [NS.kept(1, length, m * 10**7 + d) for d in (-1, 0, 1)] == [True, False, False]
        assert [NS.kept(2, length, 2 * m * 10**7 + d) for d in (-1, 0, 1)] == [True, False, False]
        assert {m * 10**7 + d for d in (-1, 0, 1)} <= set(NS.FILTER_TOTALS)
    assert all(NS.kept(f, 1, t) for f in (1, 3) for t in NS.FILTER_TOTALS + (10**15, 2**63))
    assert not any(NS.kept(f, n, 10**15) for f in (1, 1000) for n in (2, 4, 8, 16))


@pytest.mark.parametrize("kind", KINDS)
def test_filter_boundary_against_the_host_selection(kind):
    """dinth_build_dictionary_from_ngrams is the host's selection over a claimed total: around every boundary it appends what the
    model selects — the file is byte-identical — and the byte comparison does see one entry more or less"""
    gaps, _, entries = NS.boundary_collection()
    assert sorted(zip(entries["len"].tolist(), entries["freq"].tolist())) == sorted(
        [(16, 1)] + [(8, 1)] * 2 + [(4, 1)] * 4 + [(2, 1)] * 8 + [(1, 1)] * 16 + [(2, 2), (1, 2), (1, 2), (1, 3)])
    files = {}
    for total in NS.FILTER_TOTALS + (2 * 80 * 10**7 - 1, 2 * 80 * 10**7, int(gaps.size), 10**15):
        chosen = NS.select(entries, gaps, total, 65536)
        files[total] = host.pack_dictionary(kind, gaps, chosen)
        assert files[total] == host.build_dictionary_from_ngrams(kind, gaps, total, entries), total
        assert (chosen["len"] == 1).sum() == 19
    n = lambda total: len(NS.select(entries, gaps, total, 65536))
    assert [n(80 * 10**7 + d) for d in (-1, 0, 1)] == [35, 27, 27] and n(10**15) == 19 and n(int(gaps.size)) == len(entries) == 35
    assert files[80 * 10**7 - 1] != files[80 * 10**7] == files[80 * 10**7 + 1]
    assert files[2 * 80 * 10**7 - 1] != files[2 * 80 * 10**7]          # the pair of freq 2 leaves one boundary later


@pytest.mark.parametrize("kind", KINDS)
def test_a_saving_equal_to_the_threshold_is_dropped(kind):
    """NS.EXACT_TRIPLES: (9 500 000, 2, 7 599 999 999 999 999) and (868 388, 16, 6 530 277 759 999 999) have a saving that in
    double EQUALS 0.0001 / 1000, so the filter (`>`) drops them; a `>=`, or a threshold written 1e-7, would keep them. No triple
    with freq <= 1000 has this (searched here): freq * m / total is the double 1e-07 at total = 1e7 * freq * m, and one integer
    to either side moves it by 1 / total >= 1.3e-13 of itself, a thousand ulps — so the equality needs freq * m near 7e8, where
    one integer less in the total is one ulp more in the saving. The counts are set by hand: both entry points take the caller's."""
    t = 0.0001 / 1000
    assert list(NS.exact_triples(1000)) == []
    gaps, _, entries = NS.boundary_collection()
    for freq, length, total in NS.EXACT_TRIPLES:
        assert float(freq) * (48.0 * length - 16.0) / float(total) == t > 1e-7 and total < 2**53 and freq < 2**32
        assert not NS.kept(freq, length, total) and NS.kept(freq, length, total - 1) and not NS.kept(freq, length, total + 1)
        e = NS.with_freq(entries, length, freq)
        chosen = NS.select(e, gaps, total, 65536)
        assert len(chosen) == 19 and (chosen["len"] == 1).all()        # nothing else is near its boundary at such a total
        assert host.pack_dictionary(kind, gaps, chosen) == host.build_dictionary_from_ngrams(kind, gaps, total, e)
        one_more = NS.select(e, gaps, total - 1, 65536)
        assert len(one_more) == 20 and int(one_more[0]["freq"]) == freq
        assert host.pack_dictionary(kind, gaps, one_more) == host.build_dictionary_from_ngrams(kind, gaps, total - 1, e)
        assert host.pack_dictionary(kind, gaps, one_more) != host.pack_dictionary(kind, gaps, chosen)


# ---- the cases are what they are said to be -------------------------------------------------------------------------------
def test_the_cases_are_what_they_are_said_to_be():
    cases = NS.cases()
    assert tuple(cases) == NS.CASE_NAMES and max(c.gaps.size for c in cases.values()) <= 4096
    # lengths: every length, empty lists between some, a 3-letter alphabet, an odd number of chunks
    c = cases["lengths"]
    assert set(c.lens) == set(NS.LENGTHS) and c.lens.count(0) >= 5 and not c.multi and set(c.gaps.tolist()) == {0, 1, 2}
    chunks = NS.chunks_of(c.starts, False)
    assert len(chunks) == 25 and len(chunks) % 2 == 1 and sorted({n for _, n in chunks}) == sorted(
        {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 255, 256, 257 - 256, 511 - 256, 513 - 512})
    assert max(f for f, _ in c.counts.values()) > 500                  # the n-grams repeat across the lists
    # multi tails: the same lists; only the whole blocks of the 256-, 257-, 511-, 512- and 513-lists
    m = cases["multi tails"]
    assert m.multi and np.array_equal(m.gaps, c.gaps) and m.lens == c.lens
    blocks = NS.chunks_of(m.starts, True)
    assert len(blocks) == 1 + 1 + 1 + 2 + 2 and all(n == 256 for _, n in blocks)
    assert sum(f for (_, g), (f, _) in m.counts.items() if len(g) == 1) == 7 * 256 < m.total == sum(c.lens)
    none = cases["multi, no whole block"]
    assert none.multi and none.total == sum(n for n in NS.LENGTHS_LISTS if n < 256) > 0 and none.counts == {}
    # contexts: thirteen blocks that differ in one integer, every side of every boundary, six separate (0,) and (0, 0)
    x = cases["contexts"]
    assert x.multi and x.gaps.size == 13 * 256 and sum(x.lens) == x.gaps.size and all(n % 256 == 0 for n in x.lens)
    filler, zeros, pairs, seen = NS.context_filler(), {}, {}, {}
    assert set(filler.tolist()) == {0, 1} and filler[NS.CONTEXT_MAX_AT] == 0
    for b, top in enumerate(NS.CONTEXT_MAXIMA):
        block = x.gaps[b * 256:(b + 1) * 256]
        rest = np.delete(block, NS.CONTEXT_MAX_AT)
        assert int(block.max()) == top == int(block[NS.CONTEXT_MAX_AT]) and np.array_equal(rest, np.delete(filler, NS.CONTEXT_MAX_AT) * (top > 0))
        ctx = NS.CONTEXT_EDGES[top]
        assert NS.context_of(top) == ctx
        seen.setdefault(ctx, []).append(top)
        zeros[ctx] = zeros.get(ctx, 0) + int((block == 0).sum())
        pairs[ctx] = pairs.get(ctx, 0) + int(((block[0::2] == 0) & (block[1::2] == 0)).sum())
    assert seen == {0: [0, 1, M32], 1: [2, 3], 2: [4, 15], 3: [16, 255], 4: [256, 65535], 5: [65536, M32 - 1]}
    assert {k[0] for k in x.counts} == {0, 1, 2, 3, 4, 5}
    for ctx in range(6):
        assert x.counts[ctx, (0,)][0] == zeros[ctx] and x.counts[ctx, (0, 0)][0] == pairs[ctx]
    assert len({zeros[ctx] for ctx in range(6)}) > 1 and zeros[0] > zeros[1] == zeros[5] > 0
    # all distinct: 496 different n-grams in one chunk, each twice, first in the first copy
    for name in ("all distinct", "all distinct, multi"):
        a = cases[name]
        assert a.lens == [256, 256] and np.array_equal(a.gaps[:256], a.gaps[256:]) and len(set(a.gaps[:256].tolist())) == 256
        assert len(a.counts) == NS.NGRAMS_PER_CHUNK and all(f == 2 and p < 256 for f, p in a.counts.values())
        assert {k[0] for k in a.counts} == ({5} if a.multi else {0})
    # first occurrence: last n-grams of chunk 0 (ids 239 and 495: the last round of lanes 47), first in 40 later chunks
    f = cases["first occurrence"]
    assert len(NS.chunks_of(f.starts, False)) == 41 and f.lens[0] == 256
    for g in NS.FIRST_NGRAMS:
        freq, pos = f.counts[0, g]
        assert freq == 41 and pos == 256 - len(g)
        later = [p for p in range(256, f.gaps.size) if tuple(f.gaps[p:p + len(g)].tolist()) == g]
        assert len(later) >= 40 and tuple(f.gaps[pos:pos + len(g)].tolist()) == g
    assert (112 + 127) % 64 == (240 + 255) % 64 == 47
    # ties: one context; 16 single integers of one count, on both sides of 2^31; the other lengths at the same count beside them
    t = cases["ties"]
    assert not t.multi and {k[0] for k in t.counts} == {0}
    order = NS.select(t.entries, t.gaps, t.total, 65536)
    assert len(order) == len(t.entries) == 101                         # nothing is filtered at this total
    classes = [(int(e["freq"]), int(e["len"])) for e in order]
    assert [classes.count((3, n)) for n in (16, 8, 4, 2, 1)] == [1, 2, 4, 8, 16]
    at = classes.index((3, 1))
    tied = [t.ngram(e)[0] for e in order[at:at + 16]]
    assert tied == sorted(NS.TIE_VALUES) and {1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE} <= set(tied)
    assert tied != sorted(tied, key=lambda v: v - 2**32 if v >= 2**31 else v)   # a signed comparison orders them otherwise
    freqs = [f for f, _ in classes]
    assert [freqs.count(v) for v in (7, 6, 5, 3, 1)] == [3, 5, 31, 31, 31] and freqs == sorted(freqs, reverse=True)
    # the cut at 1, 2 | 7, 8 | 9: thresholds 7, 7, 6, 6, 5 — ties at 1, 2 and 7, an exact fit at 8
    assert [NS.cut_thresholds(t.entries, t.total, k)[0] for k in NS.TIE_TOP_KS] == [7, 7, 6, 6, 5]
    assert [len(NS.cut(t.entries, t.total, k)) for k in NS.TIE_TOP_KS] == [3, 3, 8, 8, 39]
    # gaps in contexts: 0, 2 and 5 only
    g = cases["gaps in contexts"]
    assert g.multi and [NS.context_of(int(g.gaps[b * 256:(b + 1) * 256].max())) for b in range(5)] == [0, 2, 5, 2, 0]
    assert {k[0] for k in g.counts} == {0, 2, 5}



def test_the_fuzz_draws_are_not_vacuous():
    draws = NS.draws()
    assert len(draws) == NS.FUZZ_DRAWS == 48 and sum(d.multi for d in draws) == 24
    assert all(d.gaps.size <= NS.FUZZ_MAX_INTS and all(0 <= n <= 600 for n in d.lens) for d in draws)
    assert all(2 <= len(d.alphabet) <= 6 and set(d.gaps.tolist()) <= set(d.alphabet) | set(NS._SPREAD) | {NS._LONELY} for d in draws)
    assert {d.top_k for d in draws} == set(NS.FUZZ_TOP_KS)
    assert all(d.gaps.size for d in draws) and any(0 in d.lens for d in draws) and any(d.multi and any(n % 256 for n in d.lens) for d in draws)
    contexts = set()
    n_cut = n_tie = n_mixed = 0
    for d in draws:
        above, tied, whole = NS.cut_profile(d.entries, d.total, d.top_k)
        n_cut += bool(above)
        n_tie += bool(tied)
        n_mixed += bool(d.multi and above - whole and whole)
        contexts |= {k[0] for k in d.counts}
    assert contexts == {0, 1, 2, 3, 4, 5}
    assert n_cut >= 16       # a context whose cut threshold is above 1
    assert n_tie >= 8        # a tie at the threshold: more than top_k of that context come back
    assert n_mixed >= 8      # multi: one context cut and another returned whole in the same call
