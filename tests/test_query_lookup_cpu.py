"""The lookups every query kernel shares (dint_amd/csrc/hip/dint_query_lookup.hpp: list_block_of, find_in_page,
find_posting) are plain C++: compiled alone with g++, they are held to numpy.searchsorted over hand-made lists — an empty
list, a one-block list, lists whose last block is short (1 and 255 docIDs), docIDs 0 and 0xFFFFFFFE — for docIDs below,
at, between and past the block maxima. The slots past a block's n hold the docID looked up: it must not be found there."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "dint_amd", "csrc", "hip", "dint_query_lookup.hpp")
SLOTS = 256
TOP = 0xFFFFFFFE  # the largest docID there is

# stdin: n_lists, then per list "fb nb"; n_blocks, then per block "n page" and its n docIDs; n_lookups, then "list d".
# stdout, per lookup: list_block_of, find_in_page in that block's page (-1: no block, or absent), find_posting (-1: absent),
# and find_in_page in the page of the list's LAST block, the one that may be short (-1: no block, or absent).
PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "%s"
using namespace dint_dev;
struct block {
    uint64_t in_off;  // (n is not the first field, as in the index's block records)
    uint32_t n;
};
int main() {
    size_t n_lists, n_blocks, n_lookups;
    if (std::scanf("%%zu", &n_lists) != 1) return 1;
    std::vector<uint32_t> first(n_lists), count(n_lists);
    for (size_t l = 0; l != n_lists; ++l)
        if (std::scanf("%%u %%u", &first[l], &count[l]) != 2) return 1;
    if (std::scanf("%%zu", &n_blocks) != 1) return 1;
    std::vector<block> blocks(n_blocks);
    std::vector<uint32_t> block_max(n_blocks), page(n_blocks), docs(n_blocks * kPageSlots);
    for (size_t b = 0; b != n_blocks; ++b) {
        if (std::scanf("%%u %%u", &blocks[b].n, &page[b]) != 2) return 1;
        for (uint32_t i = 0; i != blocks[b].n; ++i)
            if (std::scanf("%%u", &docs[size_t(page[b]) * kPageSlots + i]) != 1) return 1;
        block_max[b] = docs[size_t(page[b]) * kPageSlots + blocks[b].n - 1];
    }
    if (std::scanf("%%zu", &n_lookups) != 1) return 1;
    for (size_t x = 0; x != n_lookups; ++x) {
        uint32_t l, d;
        if (std::scanf("%%u %%u", &l, &d) != 2) return 1;
        const uint32_t fb = first[l], nb = count[l];
        for (uint32_t b = fb; b != fb + nb; ++b)  // the padding of the list's pages: the docID looked up
            for (uint32_t i = blocks[b].n; i != kPageSlots; ++i) docs[size_t(page[b]) * kPageSlots + i] = d;
        const uint32_t pos = list_block_of(block_max.data(), fb, nb, d);
        long long in_page = -1;
        if (pos < nb) {
            const uint32_t hit = find_in_page(docs.data() + size_t(page[fb + pos]) * kPageSlots, blocks[fb + pos].n, d);
            if (hit != kAbsent) in_page = hit;
        }
        const posting at = find_posting(block_max.data(), blocks.data(), fb, nb, docs.data(), d,
                                        [&](uint32_t p) { return page[fb + p]; });
        long long in_last = -1;
        if (nb) {
            const uint32_t hit = find_in_page(docs.data() + size_t(page[fb + nb - 1]) * kPageSlots, blocks[fb + nb - 1].n, d);
            if (hit != kAbsent) in_last = hit;
        }
        std::printf("%%u %%lld %%lld %%lld\n", pos, in_page, at.held() ? (long long)at.slot() : -1ll, in_last);
    }
    return 0;
}
"""

# by hand: a list is its blocks' docIDs. Between them they hold docID 0, TOP, a gap between two blocks' ranges
# (1000 .. 1999 of "short 1"), and last blocks of 1, 255 and 256 docIDs.
LISTS = {
    "one block": [[3, 9, 20, 21, 400]],
    "short 1": [list(range(0, 512, 2)), list(range(2000, 2000 + 3 * 256, 3)), [5000]],
    "empty": [],
    "short 255": [list(range(7, 7 + 256)), list(range(300, 300 + 5 * 256, 5)), list(range(TOP - 2 * 254, TOP + 1, 2))],
    "full": [list(range(1, 257)), list(range(1 << 31, (1 << 31) + 256))],
}


def lookups_of(blocks):
    """docIDs below, at, between and past what the list holds, and the two ends of the docID space"""
    ds = {0, 1, TOP, TOP - 1, 1500}
    for b in blocks:
        for d in (b[0], b[len(b) // 2], b[-1]):
            ds.update(x for x in (d - 1, d, d + 1) if 0 <= x <= TOP)
    return sorted(ds)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the lookup header"
    tmp = tmp_path_factory.mktemp("query_lookup")
    src, exe = os.path.join(tmp, "lookup.cpp"), os.path.join(tmp, "lookup")
    with open(src, "w") as f:
        f.write(PROGRAM % HEADER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__device__=", "-D__forceinline__=inline", "-o", exe, src],
                   check=True)
    names = list(LISTS)
    all_blocks = [b for name in names for b in LISTS[name]]
    pages = [len(all_blocks) - 1 - b for b in range(len(all_blocks))]  # (scattered: a block's page is not its place in the list)
    text, firsts, fb = [str(len(names))], {}, 0
    for name in names:
        firsts[name] = fb
        text.append(f"{fb} {len(LISTS[name])}")
        fb += len(LISTS[name])
    text.append(str(len(all_blocks)))
    for b, docs in enumerate(all_blocks):
        assert 0 < len(docs) <= SLOTS and docs == sorted(set(docs))
        text.append(f"{len(docs)} {pages[b]} " + " ".join(map(str, docs)))
    # every list is asked for its own docIDs of interest and for every other list's
    lookups = [(l, d) for l, name in enumerate(names) for other in names for d in lookups_of(LISTS[other])]
    text.append(str(len(lookups)))
    text += [f"{l} {d}" for l, d in lookups]
    out = subprocess.run([exe], input="\n".join(text), check=True, capture_output=True, text=True).stdout.split("\n")
    got = [tuple(int(x) for x in line.split()) for line in out if line]
    assert len(got) == len(lookups)
    return [(names[l], LISTS[names[l]], pages[firsts[names[l]]:], d, g) for (l, d), g in zip(lookups, got)]


def place(docs, d):
    """where d is among docs, by numpy.searchsorted (-1: absent)"""
    a = np.array(docs, dtype=np.uint64)
    hit = int(np.searchsorted(a, np.uint64(d), side="left"))
    return hit if hit != len(a) and int(a[hit]) == d else -1


def expected(blocks, pages, d):
    """(list_block_of, find_in_page, find_posting, find_in_page in the last block) by numpy.searchsorted"""
    pos = int(np.searchsorted(np.array([b[-1] for b in blocks], dtype=np.uint64), np.uint64(d), side="left"))
    in_last = place(blocks[-1], d) if blocks else -1
    hit = place(blocks[pos], d) if pos != len(blocks) else -1
    return pos, hit, pages[pos] * SLOTS + hit if hit != -1 else -1, in_last


def test_every_lookup_agrees_with_searchsorted(cases):
    for name, blocks, pages, d, got in cases:
        assert got == expected(blocks, pages, d), (name, d)


def test_the_cases_the_lookups_must_handle_are_among_them(cases):
    seen = {(name, d): got[:3] for name, _, _, d, got in cases}
    last = {(name, d): got[3] for name, _, _, d, got in cases}
    assert all(got == (0, -1, -1) for (name, _), got in seen.items() if name == "empty")  # nb == 0: past the last docID
    assert seen[("one block", 400)][:2] == (0, 4) and seen[("one block", 401)] == (1, -1, -1)
    assert seen[("one block", 2)] == (0, -1, -1)  # below the first docID
    assert seen[("short 1", 0)][:2] == (0, 0) and seen[("one block", 0)] == (0, -1, -1)  # d = 0, held and not
    assert seen[("short 1", 510)][:2] == (0, 255)  # a block maximum
    assert seen[("short 1", 1500)] == (1, -1, -1)  # between two blocks' ranges
    assert seen[("short 1", 5000)][:2] == (2, 0) and seen[("short 1", 5001)] == (3, -1, -1)  # n = 1, and past the last maximum
    # the padding holds the docID looked up: past a short block's n it is not found
    assert last[("short 1", 5000)] == 0 and last[("short 1", 5001)] == -1 and last[("short 1", TOP)] == -1
    assert last[("short 255", TOP)] == 254 and last[("one block", 401)] == -1 and last[("one block", TOP)] == -1
    assert seen[("short 255", TOP)][:2] == (2, 254) and seen[("short 255", TOP - 1)] == (2, -1, -1)  # n = 255, d = 0xFFFFFFFE
    assert seen[("full", TOP)] == (2, -1, -1)
