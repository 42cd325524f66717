"""The staged input layouts of the query calls (dint_amd/csrc/hip/host/hip_stage_layout.inc) are plain C++: compiled
alone with g++, two of them are checked against offsets written out by hand from the expressions the calls used before the
layouts had one description each — `(2 * n_pages + 2 * n_tab + 31) / 32 * 32` and so on — for an odd and an even count.
The two schedule workspaces of the decode launch live there too (byte offsets): checked the same way, given the three kernel
constants they are sized by as read out of the kernel headers."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = os.path.join(ROOT, "dint_amd", "csrc", "hip", "host", "hip_stage_layout.inc")

HIP = os.path.join(ROOT, "dint_amd", "csrc", "hip")


def kernel_constants():
    """kChunkUnits, kQueueStride and kQueueLines (= kQueueShards + 1 + kChunkShards) as the kernel headers define them"""
    text = open(os.path.join(HIP, "dint_kernels.hpp")).read() + open(os.path.join(HIP, "kernels", "bundles.inc")).read()
    value = {}
    for name in ("kChunkUnits", "kQueueStride", "kQueueShards", "kChunkShards"):
        (v,) = re.findall(r"constexpr uint32_t %s = (\d+);" % name, text)
        value[name] = int(v)
    assert re.search(r"constexpr uint32_t kQueueLines = kQueueShards \+ 1 \+ kChunkShards;", text)
    value["kQueueLines"] = value["kQueueShards"] + 1 + value["kChunkShards"]
    return value


PROGRAM = r"""
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "%s"
constexpr size_t kChunkUnits = %d, kCounterBytes = size_t(%d) * %d * 4;  // (a launch's kQueueLines lines of kQueueStride words)
int main() {
    const size_t ctrl_words = 320, step_bytes = 204;  // (step_bytes: not a multiple of 8, 52 words a step)
    for (int even = 0; even != 2; ++even) {
        const and_general_layout a = even ? and_general_layout(40, 1, 1, 1, ctrl_words, step_bytes)
                                          : and_general_layout(3, 6, 3, 2, ctrl_words, step_bytes);
        std::printf("and %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", a.page_block, a.page_query, a.term_first, a.term_blocks, a.ctrl,
                    a.counts, a.steps, a.words);
        const maxscore_layout m = even ? maxscore_layout(4, 1, 2, 0) : maxscore_layout(5, 2, 3, 1);
        std::printf("maxscore %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", m.term_first,
                    m.term_blocks, m.term_page, m.term_claimed, m.term_weight, m.term_order, m.term_e, m.rec_query, m.q_from, m.q_n,
                    m.q_ne, m.q_theta, m.cpage_page, m.cpage_rec, m.rest_blocks, m.q_rest, m.q_margin, m.words);
    }
    for (size_t n : {size_t(1), size_t(300)}) {
        const sched_layout l(n, kChunkUnits);
        std::printf("sched %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", l.urec, l.cbase, l.items, l.block, l.n_items, l.sch, l.item_cnt, l.need);
    }
    for (size_t n : {size_t(1), size_t(33)}) {
        const split_layout l(n, kChunkUnits, kCounterBytes);
        std::printf("split %%zu %%zu %%zu %%zu %%zu %%zu %%zu %%zu\n", l.urec, l.cbase, l.end, l.left, l.n_left, l.clock, l.counters, l.need);
    }
    uint32_t area[8] = {};
    if (at_byte<uint32_t>(area, 12) != area + 3) return 1;
    return staged<uint64_t>(area, 2) == reinterpret_cast<uint64_t*>(area + 2) ? 0 : 1;  // one offset, any base
}
"""

# by hand. AND general form, 3 pages, 2 rounds x 3 queries: tables 3 + 3 + 6 + 6 = 18 -> 32; counters (2 + 1) * 320 = 960
# and 2 * 3 result words, 966; steps (2 + 1) * 52 = 156. 40 pages, 1 round x 1 query: 40 + 40 + 1 + 1 = 82 -> 96; 640 + 2; 104.
AND_ODD = [0, 3, 6, 12, 32, 992, 998, 1154]
AND_EVEN = [0, 40, 80, 81, 96, 736, 738, 842]
# the pruned ranked call's main stage, 5 records, 2 queries, 3 candidate pages, 1 other E block: 40 + 8 + 6 + 1 = 55 -> 56,
# then 2 x 2 doubles. 4 records, 1 query, 2 candidate pages, no other E block: 32 + 4 + 4 = 40, then 2 doubles.
MAXSCORE_ODD = [0, 5, 10, 15, 20, 25, 30, 35, 40, 42, 44, 46, 48, 51, 54, 56, 60, 64]
MAXSCORE_EVEN = [0, 4, 8, 12, 16, 20, 24, 28, 32, 33, 34, 35, 36, 38, 40, 40, 42, 44]
# A bundle schedule's workspace, in bytes, from `need = 16 * n_units + 16 * n_chunks + 4 * n_units + 4 * n_blocks + 4 + 2 * n_units`
# and the pointer chain behind it (records, chunk bases, items, block counts, n_items, schedule bytes, item counts), chunks of
# 64 units, blocks of 256. 1 unit: 1 chunk, 1 block: 16, +16, +4, +4, +4, +1, +1. 300 units: 5 chunks, 2 blocks: 4800, +80,
# +1200, +8, +4, +300, +300.
SCHED_1 = [0, 16, 32, 36, 40, 44, 45, 46]
SCHED_300 = [0, 4800, 4880, 6080, 6088, 6092, 6392, 6692]
# The cut units' workspace, from `need = 16 * n_sub + 16 * n_chunks + 8 * n_sub + 4 * n_items + 256 + kQueueLines * kQueueStride * 4`
# (n_sub = 2 * n_items; 41 counter lines of 128 bytes = 5248): records, chunk bases, end offsets, left items, n_left (the cut
# units' clock word 2 words behind it), the counters a 256-byte line behind n_left. 1 item: 2 records, 1 chunk: 32, +16, +16,
# +4, then 68 + 256 = 324 and 324 + 5248. 33 items: 66 records, 2 chunks: 1056, +32, +528, +132, then 1748 + 256 and + 5248.
SPLIT_1 = [0, 32, 48, 64, 68, 76, 324, 5572]
SPLIT_33 = [0, 1056, 1088, 1616, 1748, 1756, 2004, 7252]


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the layout helper"
    d = tmp_path_factory.mktemp("stage_layout")
    src, exe = os.path.join(d, "layouts.cpp"), os.path.join(d, "layouts")
    with open(src, "w") as f:
        k = kernel_constants()
        f.write(PROGRAM % (LAYOUTS, k["kChunkUnits"], k["kQueueLines"], k["kQueueStride"]))
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    return [[int(x) for x in line.split()[1:]] for line in out if line]


def test_the_and_general_form_is_laid_out_as_before(printed):
    assert printed[0] == AND_ODD
    assert printed[2] == AND_EVEN
    for row in (printed[0], printed[2]):
        assert row[5] % 2 == 0 and row[6] % 2 == 0  # the result counters and the steps hold 8-byte values


def test_the_maxscore_main_stage_is_laid_out_as_before(printed):
    assert printed[1] == MAXSCORE_ODD
    assert printed[3] == MAXSCORE_EVEN
    for row in (printed[1], printed[3]):
        assert row[15] % 2 == 0 and row[16] % 2 == 0  # rest and margin are doubles


def test_the_schedule_workspaces_are_laid_out_as_before(printed):
    k = kernel_constants()
    assert (k["kChunkUnits"], k["kQueueLines"], k["kQueueStride"]) == (64, 41, 32)  # what the numbers by hand assume
    assert printed[4:8] == [SCHED_1, SCHED_300, SPLIT_1, SPLIT_33]
    for row in (SCHED_1, SCHED_300):
        assert row[1] % 16 == 0 and row[2] % 4 == 0 and row[3] % 4 == 0 and row[4] % 4 == 0  # 16-byte records and bases, u32 fields
    for row in (SPLIT_1, SPLIT_33):
        assert row[1] % 16 == 0 and row[2] % 8 == 0 and row[3] % 4 == 0 and row[4] % 4 == 0 and row[6] % 4 == 0
