"""The staged input layouts of the query calls (dint_amd/csrc/hip/host/hip_stage_layout.inc) are plain C++: compiled
alone with g++, two of them are checked against offsets written out by hand from the expressions the calls used before the
layouts had one description each — `(2 * n_pages + 2 * n_tab + 31) / 32 * 32` and so on — for an odd and an even count."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = os.path.join(ROOT, "dint_amd", "csrc", "hip", "host", "hip_stage_layout.inc")

PROGRAM = r"""
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include "%s"
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
    uint32_t area[8] = {};
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


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the layout helper"
    d = tmp_path_factory.mktemp("stage_layout")
    src, exe = os.path.join(d, "layouts.cpp"), os.path.join(d, "layouts")
    with open(src, "w") as f:
        f.write(PROGRAM % LAYOUTS)
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
