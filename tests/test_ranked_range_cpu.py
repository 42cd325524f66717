"""DocID-range ranked queries without a GPU: the two entries in the header, the library and the
binding; the model (tests/ranked_range.py) against a brute-force filter of the union / the intersection; the tiling property
— the merged top-k of slices that tile the docID space is the unranged top-k; list_blocks_in_range of
dint_query_lookup.hpp, compiled alone with g++, against numpy.searchsorted; and the batch of tests/test_gpu_ranked_range.py
shown not to be vacuous on the three corpora."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import ranked
import ranked_or
import ranked_range as RR
from dint_amd import host
from queries import heavy_queries, reference_queries
from test_index_cpu import get_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "dint_amd", "csrc", "hip", "dint_query_lookup.hpp")
CORPORA = ["small_corpus", "dense_corpus", "sparse_corpus"]
ENTRIES = ("dint_ranked_or_range_queries", "dint_ranked_and_range_queries")


def _setup(ix):
    num_docs = int(ix.docids.max()) + 1
    nl = ranked.norm_lens(host.sizes_from_postings(ix.docids, ix.freqs, num_docs))
    return ranked.BuilderLists(ix.docids, ix.freqs, ix.bounds), nl, num_docs


def bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_the_entries_are_declared_exported_and_bound():
    from dint_amd import device

    header = open(os.path.join(ROOT, "include", "dint_hip.h")).read()
    assert device.abi_version() == 6 and "#define DINT_ABI_VERSION 6" in header
    assert "typedef struct dint_doc_range" in header
    for name in ENTRIES:
        assert f"int {name}(" in header
        assert name in device.ABI_SYMBOLS and hasattr(device._lib, name)
        assert hasattr(device.QueryIndex, name[len("dint_"):])


def test_argument_errors_need_no_device():
    import ctypes as C

    from dint_amd import device

    counts = np.full(1, 77, dtype=np.uint64)
    scores = np.zeros(2048, dtype=np.float32)
    terms = np.zeros(1, dtype=np.uint32)
    offs = np.array([0, 1], dtype=np.uint64)
    blocks = C.c_uint64(77)
    fake = C.c_void_p(8)  # (never dereferenced: the null arguments and a bad k are refused first)
    for name in ENTRIES:
        call = getattr(device._lib, name)
        for qi, fd, w, k, cnt in ((None, fake, fake, 10, counts), (fake, None, fake, 10, counts), (fake, fake, None, 10, counts),
                                  (fake, fake, fake, 0, counts), (fake, fake, fake, 1025, counts), (fake, fake, fake, 10, None)):
            assert call(qi, fd, w, k, terms.ctypes.data, offs.ctypes.data, None, 1, cnt.ctypes.data if cnt is not None else None, None,
                        scores.ctypes.data, None, C.byref(blocks), None) == -1
            assert counts[0] == 77 and blocks.value == 77 and not scores.any()  # nothing is written


@pytest.mark.parametrize("conjunctive", [False, True])
def test_the_model_is_a_brute_force_filter(small_corpus, conjunctive):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    qs, ranges = RR.ranged_batch(reference_queries(len(ix.lens))[::7] + heavy_queries(ix.lens, 10), num_docs)
    model = ranked.ranked_and if conjunctive else ranked_or.ranked_or
    seen = 0
    for q, own in zip(qs, ranges.tolist()):
        sets = [set(lists.postings(int(t))[0].tolist()) for t in q]
        docs = (set.intersection(*sets) if conjunctive else set.union(*sets)) if sets else set()
        # the unranged model's own scores of exactly those documents
        full = model(lists, q, nl, num_docs, max(1, len(docs)))
        score_of = dict(zip(full[2][:full[0]].tolist(), bits(full[1][:full[0]]).tolist()))
        assert set(score_of) == docs
        every = RR.every_match(lists, q, nl, num_docs, conjunctive)
        for lo, hi in [tuple(own)] + RR.slices(0, num_docs, 2):  # (the query's range of the batch, and the two halves)
            inside = sorted(d for d in docs if lo <= d < hi)
            n, sc, ids, matches = RR.top_in_range(every, lo, hi, 10)
            assert matches == len(inside) and n == min(10, matches)
            order = sorted(inside, key=lambda d: (-float(np.uint32(score_of[d]).view(np.float32)), d))[:10]
            assert ids[:n].tolist() == order and bits(sc[:n]).tolist() == [score_of[d] for d in order]
            assert (ids[n:] == 0xFFFFFFFF).all() and not sc[n:].any()
            seen += matches
    assert seen > 500


@pytest.mark.parametrize("s", [1, 2, 3, 7])
@pytest.mark.parametrize("conjunctive", [False, True])
def test_slices_that_tile_the_docid_space_merge_to_the_unranged_answer(small_corpus, conjunctive, s):
    ix = get_index(small_corpus, host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    model = ranked.ranked_and if conjunctive else ranked_or.ranked_or
    for q in reference_queries(len(ix.lens))[::9] + heavy_queries(ix.lens, 6):
        every = RR.every_match(lists, q, nl, num_docs, conjunctive)
        for k in (1, 10, 1000):
            parts = [RR.top_in_range(every, lo, hi, k) for lo, hi in RR.slices(0, num_docs, s)]
            n, sc, ids = RR.merge_topk(parts, k)
            want = model(lists, q, nl, num_docs, k)
            assert n == want[0] and np.array_equal(bits(sc), bits(want[1])) and np.array_equal(ids, want[2])
            assert sum(p[3] for p in parts) == every[1].size


@pytest.mark.parametrize("corpus_name", CORPORA)
def test_the_gpu_batch_is_not_vacuous(request, corpus_name):
    ix = get_index(request.getfixturevalue(corpus_name), host.SINGLE_PACKED)
    lists, nl, num_docs = _setup(ix)
    qs, ranges = RR.ranged_batch(reference_queries(len(ix.lens)) + heavy_queries(ix.lens, 60), num_docs)
    assert len(ranges) == len(qs) and len(set(map(tuple, ranges.tolist()))) > len(qs) // 2
    widths = ranges[:, 1].astype(np.int64) - ranges[:, 0]
    assert widths.min() == 1 and widths.max() >= num_docs
    for conjunctive in (False, True):  # (the matches are the sets' own: no scores needed here)
        total = 0
        for q, (lo, hi) in zip(qs, ranges.tolist()):
            docs = [lists.postings(int(t))[0] for t in q]
            d = functools.reduce(np.intersect1d if conjunctive else np.union1d, docs).astype(np.int64) if docs else np.zeros(0, np.int64)
            total += int(((d >= lo) & (d < hi)).sum())
        assert total > 500, (conjunctive, total)
    # the same terms under different ranges
    assert qs[-12:] == [list(q) for q in qs[:12]] and (ranges[-12:] != ranges[:12]).any(axis=1).all()


PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "%s"
using namespace dint_dev;
int main() {
    size_t nb, n;
    if (std::scanf("%%zu", &nb) != 1) return 1;
    std::vector<uint32_t> maxima(nb);
    for (auto& m : maxima)
        if (std::scanf("%%u", &m) != 1) return 1;
    if (std::scanf("%%zu", &n) != 1) return 1;
    for (size_t i = 0; i != n; ++i) {
        uint32_t lo, hi;
        if (std::scanf("%%u %%u", &lo, &hi) != 2) return 1;
        const block_span s = list_blocks_in_range(maxima.data(), uint32_t(nb), lo, hi);
        std::printf("%%u %%u %%u\n", s.p0, s.p1, s.size());
    }
    return 0;
}
"""

TOP = 0xFFFFFFFE
MAXIMA = {0: [], 1: [400], 2: [255, 5000], 5: [510, 2765, 5000, 1 << 31, TOP]}


def _ranges_of(maxima):
    """lo and hi - 1 below the first maximum, at a maximum, one above a maximum and above the last; lo >= hi"""
    points = {0, 1, 7, TOP, TOP + 1}
    for m in maxima:
        points.update(x for x in (m - 1, m, m + 1) if 0 <= x <= TOP + 1)
    points = sorted(points)
    out = [(lo, last + 1) for lo in points for last in points if lo <= last <= TOP]  # hi - 1 = last
    out += [(lo, hi) for lo in points for hi in points if lo >= hi]                  # empty, and inverted
    return out


@pytest.fixture(scope="module")
def span_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the lookup header"
    tmp = tmp_path_factory.mktemp("block_span")
    src, exe = os.path.join(tmp, "span.cpp"), os.path.join(tmp, "span")
    with open(src, "w") as f:
        f.write(PROGRAM % HEADER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__device__=", "-D__forceinline__=inline", "-o", exe, src],
                   check=True)
    return exe


@pytest.mark.parametrize("nb", sorted(MAXIMA))
def test_list_blocks_in_range_agrees_with_searchsorted(span_exe, nb):
    maxima = MAXIMA[nb]
    ranges = _ranges_of(maxima)
    text = [str(nb), " ".join(map(str, maxima)), str(len(ranges))] + [f"{lo} {hi}" for lo, hi in ranges]
    out = subprocess.run([span_exe], input="\n".join(text), check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(int(x) for x in line.split()) for line in out if line]
    assert len(got) == len(ranges)
    some = 0
    for (lo, hi), (p0, p1, size) in zip(ranges, got):
        want = RR.blocks_in_range(maxima, lo, hi)
        assert (p0, p1) == want and size == p1 - p0 and 0 <= p0 <= p1 <= nb, (maxima, lo, hi)
        if lo >= hi:
            assert size == 0
        else:  # the positional rule is the record rule: max >= lo and base < hi, a block's base one past the block before's max
            bases = [0] + [m + 1 for m in maxima[:-1]]
            assert [p for p in range(nb) if maxima[p] >= lo and bases[p] < hi] == list(range(p0, p1))
        some += size
    assert some > 0 or nb == 0
