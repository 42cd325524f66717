"""The stream touch of the vroom single-dictionary segments (kernels/segment.inc, TOUCH; dint_stream_touch.hpp), without a GPU.

* The window rule — stream_touch(in_off, n, enc_bytes, max_lanes) -> (first line, lanes) — compiled alone with g++
  (tests/cpp/stream_touch_cases.cpp) against a model written out here from the header's description, and against the
  bounds themselves: lane l < lanes reads the four bytes at first_line + 128 l, and none of them may lie at or past enc_bytes.
* The build: decode_single_kernel keeps tests/test_kernel_build_cpu.py's ceilings (at most 128 vector registers, none spilled, no
  scratch) with the touch compiled in, and every in-index, pair and query decode kernel has the spill counts of a build with
  -DDINT_STREAM_TOUCH_LANES=0: the touch is gated at compile time and is the vroom launches' alone."""
import importlib.util
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

LINE = 128
PROLOGUE = 3 * 512  # the bytes of tiles 0, 1 and 2
# n integers are taken for n * 19 // 32 stream bytes (dint_stream_touch.hpp): the prologue's 1536 bytes cover a unit up to ...
NO_TOUCH_N = max(n for n in range(2000, 3000) if n * 19 // 32 <= PROLOGUE)


def model(in_off, n, enc_bytes, cap):
    """The rule as the header describes it, in Python's unbounded integers."""
    tile3 = in_off + PROLOGUE
    if tile3 >= enc_bytes:
        return 0, 0
    est = min(n, 1 << 20) * 19 // 32
    if est <= PROLOGUE:
        return 0, 0
    line = tile3 // LINE * LINE
    want = -(-(tile3 - line + est - PROLOGUE) // LINE)
    fit = (enc_bytes - line - 4) // LINE + 1 if enc_bytes - line >= 4 else 0
    lanes = min(want, cap, fit)
    return (line, lanes) if lanes else (0, 0)


@pytest.fixture(scope="module")
def touch_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the window rule"
    exe = os.path.join(tmp_path_factory.mktemp("stream_touch"), "cases")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/dint_amd/csrc/hip", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "stream_touch_cases.cpp")], check=True)
    return exe


def run(exe, cases):
    text = "\n".join(" ".join(map(str, c)) for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    got = [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(len(cases))]
    assert len(out) == 2 * len(cases)
    return got


def check(exe, cases):
    got = run(exe, cases)
    for (in_off, n, enc_bytes, cap), (line, lanes) in zip(cases, got):
        what = (in_off, n, enc_bytes, cap, line, lanes)
        assert (line, lanes) == model(in_off, n, enc_bytes, cap), what
        assert lanes <= cap and line % LINE == 0 and line < enc_bytes, what  # (no lanes: line 0, and the host takes no stream below 8 bytes)
        if lanes:
            assert line == (in_off + PROLOGUE) // LINE * LINE, what       # the line that holds tile 3's first byte
            assert line + LINE * (lanes - 1) + 4 <= enc_bytes, what      # the last lane's dword ends inside the stream
    return got


BIG = 1 << 40  # a stream no window reaches the end of


def test_the_threshold_below_which_the_prologue_covers_the_unit(touch_exe):
    assert 2400 < NO_TOUCH_N < 2800  # "about 2700" at 0.56 bytes an integer; 2588 with the rule's 19 / 32
    ns = [1, 255, 256, NO_TOUCH_N - 1, NO_TOUCH_N, NO_TOUCH_N + 1, NO_TOUCH_N + 2, 3000]
    got = check(touch_exe, [(in_off, n, BIG, 64) for n in ns for in_off in (0, 1, 127)])
    for (n, in_off), (_, lanes) in zip([(n, o) for n in ns for o in (0, 1, 127)], got):
        assert (lanes == 0) == (n <= NO_TOUCH_N), (n, in_off, lanes)
    assert run(touch_exe, [(0, NO_TOUCH_N + 1, BIG, 64)]) == [(PROLOGUE, 1)]  # one byte behind tile 2: one line


@pytest.mark.parametrize("cap", [0, 16, 32, 64])
def test_a_unit_of_16384_integers_takes_the_full_cap_and_shorter_ones_less(touch_exe, cap):
    got = check(touch_exe, [(in_off, 16384, BIG, cap) for in_off in (0, 1, 127, 128, 5000)])
    assert [lanes for _, lanes in got] == [cap] * 5
    assert [line for line, _ in got] == ([0] * 5 if cap == 0 else [1536, 1536, 1536, 1664, 6528])
    # the window grows with n and stops at the cap; n past any unit the host accepts changes nothing
    ns = [3000, 4096, 8192, 12000, 16383, 16384, 65536, 1 << 28, (1 << 32) - 1]
    lanes = [l for _, l in check(touch_exe, [(64, n, BIG, cap) for n in ns])]
    assert lanes == sorted(lanes) and lanes[-1] == cap and (cap == 0 or 0 < lanes[0] <= 3)
    if cap == 64:
        assert lanes[2] == (8192 * 19 // 32 - PROLOGUE + 64 + 127) // 128  # half a unit: 27 lines


def test_line_offsets_of_the_units_first_byte(touch_exe):
    got = check(touch_exe, [(1 << 20 | off, 8192, BIG, 64) for off in (0, 1, 63, 64, 126, 127)])
    assert {line for line, _ in got} == {(1 << 20) + PROLOGUE}
    assert [l for _, l in got] == [26, 27, 27, 27, 27, 27]  # 3328 bytes (26 lines) behind tile 2, from `off` bytes into the line


def test_the_streams_end(touch_exe):
    """Tile 3 begins in the stream's last line, exactly at its end, past it; the last lane's dword against the end byte by byte."""
    cases = []
    for in_off in (0, 1, 127, 128 * 77 + 5):
        tile3 = in_off + PROLOGUE
        line = tile3 // LINE * LINE
        for enc_bytes in range(max(8, tile3 - 3), tile3 + 2 * LINE + 6):  # from "past the end" through the last line into the next two
            cases.append((in_off, 16384, enc_bytes, 64))
        # every count of whole lines that still fit, the end one byte short of / at / past the next lane's dword
        for k in (1, 2, 15, 16, 17, 63, 64, 65):
            for d in (3, 4, 5):
                cases.append((in_off, 16384, line + LINE * (k - 1) + d, 64))
    got = check(touch_exe, cases)
    for (in_off, _, enc_bytes, _), (line, lanes) in zip(cases, got):
        tile3 = in_off + PROLOGUE
        if tile3 >= enc_bytes:
            assert (line, lanes) == (0, 0), (in_off, enc_bytes)             # at the end and past it: nothing
        elif enc_bytes <= tile3 // LINE * LINE + LINE:
            assert lanes <= 1, (in_off, enc_bytes)                          # in the stream's last line: that line at the most
    assert any(l == 1 for _, l in got) and any(l == 64 for _, l in got) and any(l == 63 for _, l in got)
    # a unit that begins past the stream's end (a table the device does not trust): nothing, whatever n
    assert run(touch_exe, [(1000, 16384, 999, 64), ((1 << 64) - 1, 16384, 1 << 20, 64), ((1 << 64) - 1536, 16384, (1 << 64) - 1, 64)]) == [(0, 0)] * 3


def test_offsets_around_4_gib_are_64_bit(touch_exe):
    cases = [((1 << 32) + d, 16384, (1 << 32) + end, 64) for d in (-1537, -1536, -1535, -130, -1, 0, 1, 127)
             for end in (-1, 0, 1, 4, 200, 4096, 1 << 20)]
    cases += [((1 << 33) - 1, 16384, 1 << 34, 64), ((1 << 47) + 3, 9000, (1 << 47) + 4000, 64)]
    got = check(touch_exe, cases)
    assert sum(1 for line, lanes in got if lanes and line >= 1 << 32) >= 8      # windows wholly above 2^32 ...
    assert sum(1 for line, lanes in got if lanes and line < 1 << 32 <= line + LINE * lanes) >= 2  # ... and across it
    assert run(touch_exe, [((1 << 32) - 1536, 16384, (1 << 32) + 4096, 64)]) == [(1 << 32, 32)]  # (4096 - 4) // 128 + 1


def test_the_smallest_stream(touch_exe):
    got = check(touch_exe, [(in_off, n, 8, cap) for in_off in (0, 1, 7, 8, 9) for n in (1, 4, 16384, 1 << 28) for cap in (0, 64)])
    assert set(got) == {(0, 0)}


# ---- the build -----------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("check_inflight", os.path.join(ROOT, "tools", "check_inflight.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_touch_costs_no_spill_and_leaves_the_other_kernels_alone(tmp_path):
    tool = _tool()
    with ThreadPoolExecutor(2) as pool:  # (two cross-compiles of ~25 s, side by side)
        shipped = pool.submit(tool.compile_to_asm, str(tmp_path / "shipped"))
        without = pool.submit(tool.compile_to_asm, str(tmp_path / "without"), ("-DDINT_STREAM_TOUCH_LANES=0",))
        shipped, without = tool.kernel_resources(shipped.result()), tool.kernel_resources(without.result())
    assert shipped.keys() == without.keys()
    single = [k for k in shipped if "dint_dev20decode_single_kernelE" in k]
    assert len(single) == 1
    for res in (shipped, without):
        r = res[single[0]]
        assert r["vgpr_count"] <= 128 and r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    others = [k for k in shipped if "decode_" in k and any(w in k for w in ("index", "pair", "query"))]
    assert len(others) >= 12, others
    for k in others:
        for field in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
            assert shipped[k][field] == without[k][field], (k, field, shipped[k], without[k])
