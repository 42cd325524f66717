"""The window of a unit whose byte span is known (dint_stream_touch.hpp: stream_touch_span, unit_stream_span, unit_touch), without
a GPU.

* stream_touch_span(in_off, span, enc_bytes, max_lines, past) -> (first line, lines), compiled alone with g++
  (tests/cpp/stream_touch_span_cases.cpp), against a model written out here in Python's unbounded integers and against the bounds
  themselves: line l < lines is touched by the four bytes at first_line + 128 l, none of them at or past enc_bytes, no line
  behind the one that holds the byte `past` behind the unit's last, at most max_lines.
* unit_stream_span: what decode_unit_single takes for a unit's span — up to the next record, the stream's end for the last
  record, not known (0) where the next record begins at or before this one; cut to 6 n bytes, saturated to 32 bits.
* unit_touch: a span that is not known falls back to the rule of n, stream_touch, exactly.
* The build: decode_single_kernel with the span and the second load has no more spilled scalar registers than the build before
  them had (56), within tests/test_kernel_build_cpu.py's ceilings."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

LINE = 128
PROLOGUE = 3 * 512  # the bytes of tiles 0, 1 and 2
U32 = (1 << 32) - 1
BIG = 1 << 40       # a stream no window reaches the end of
CAPS = (0, 64, 96, 128)
PASTS = (0, 1536)


def model(in_off, span, enc_bytes, cap, past):
    """The lines from the one of tile 3's first byte through the one of the byte `past` behind the unit's last."""
    tile3 = in_off + PROLOGUE
    if tile3 >= enc_bytes or span <= PROLOGUE:
        return 0, 0
    line = tile3 // LINE * LINE
    last_byte = in_off + span + past - 1
    want = last_byte // LINE - line // LINE + 1
    fit = (enc_bytes - line - 4) // LINE + 1 if enc_bytes - line >= 4 else 0
    lines = min(want, cap, fit)
    return (line, lines) if lines else (0, 0)


def old_model(in_off, n, enc_bytes, cap=64):
    """stream_touch, as tests/test_stream_touch_cpu.py writes it out."""
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


def span_model(in_off, n, has_next, next_in_off, enc_bytes):
    end = next_in_off if has_next else enc_bytes
    if end <= in_off:
        return 0
    return min(end - in_off, 6 * n, U32)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to compile the window rule"
    path = os.path.join(tmp_path_factory.mktemp("stream_touch_span"), "cases")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{ROOT}/dint_amd/csrc/hip", "-o", path,
                    os.path.join(ROOT, "tests", "cpp", "stream_touch_span_cases.cpp")], check=True)
    return path


def run(exe, kind, cases):
    text = "\n".join(kind + " " + " ".join(map(str, c)) for c in cases)
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.split()
    per = 1 if kind == "s" else 2
    assert len(out) == per * len(cases)
    vals = list(map(int, out))
    return vals if per == 1 else [(vals[2 * i], vals[2 * i + 1]) for i in range(len(cases))]


def check(exe, cases):
    """cases: (in_off, span, enc_bytes, cap, past)."""
    got = run(exe, "w", cases)
    for (in_off, span, enc_bytes, cap, past), (line, lines) in zip(cases, got):
        what = (in_off, span, enc_bytes, cap, past, line, lines)
        assert (line, lines) == model(in_off, span, enc_bytes, cap, past), what
        assert lines <= cap and line % LINE == 0, what
        if lines:
            assert line == (in_off + PROLOGUE) // LINE * LINE, what               # the line that holds tile 3's first byte
            assert line + LINE * (lines - 1) + 4 <= enc_bytes, what              # the last line's dword ends inside the stream
            assert line + LINE * (lines - 1) <= in_off + span + past - 1, what   # no line behind the unit's last byte (+ past)
        else:
            assert line == 0, what
    return got


def filling(in_off, k):
    """The largest span whose window (past 0) is exactly k lines: the unit's last byte is the last byte of line k - 1."""
    line = (in_off + PROLOGUE) // LINE * LINE
    return line + LINE * k - in_off


def test_spans_that_the_prologue_covers(exe):
    got = check(exe, [(in_off, span, BIG, cap, 0) for in_off in (0, 1, 127) for span in (0, 1, PROLOGUE, PROLOGUE + 1) for cap in CAPS])
    for (in_off, span, _, cap, _), (_, lines) in zip([(i, s, 0, c, 0) for i in (0, 1, 127) for s in (0, 1, PROLOGUE, PROLOGUE + 1) for c in CAPS], got):
        assert lines == (1 if span == PROLOGUE + 1 and cap else 0), (in_off, span, cap)
    # ... but `past` counts only for a unit that has a window of its own
    assert run(exe, "w", [(0, PROLOGUE, BIG, 128, 1536), (0, PROLOGUE + 1, BIG, 128, 1536)]) == [(0, 0), (PROLOGUE, 13)]


@pytest.mark.parametrize("past", PASTS)
@pytest.mark.parametrize("cap", CAPS)
def test_spans_that_fill_64_and_128_lines(exe, cap, past):
    """One load against two, and the cap: the span at, one below and one above the byte count that fills exactly 64 and exactly
    128 lines (and the smallest span that needs the 64th / 128th line), unit starts at residues 0, 1 and 127 of a line."""
    cases, expect = [], []
    for in_off in (0, 1, 127, 128 * 1000 + 1, 128 * 1000 + 127):
        for k in (64, 128):
            full = filling(in_off, k)
            for span, lines in ((full - 128, k - 1), (full - 127, k), (full - 1, k), (full, k), (full + 1, k + 1)):
                cases.append((in_off, span, BIG, cap, past))
                expect.append(min(lines + past // LINE, cap))
    got = check(exe, cases)
    assert [lines for _, lines in got] == expect
    if cap == 128 and past == 0:
        assert {64, 65, 127, 128} <= set(expect)  # either side of the second load's first line, and of the cap


def test_the_window_follows_the_span_not_n(exe):
    # the bench stream's long units span 5.7 to 17 KB: 33 to 124 lines behind tile 2, none behind their end
    for span, lines in ((5700, 33), (7600, 48), (9900, 66), (13800, 96), (17100, 122), (17500, 125), (32768, 128)):
        assert run(exe, "w", [(0, span, BIG, 128, 0)]) == [(PROLOGUE, lines)], span
    got = check(exe, [(in_off, span, BIG, 128, 0) for in_off in (0, 77, 5000) for span in range(1500, 20000, 37)])
    lines = [l for _, l in got[:500]]
    assert lines == sorted(lines)


def test_the_streams_end(exe):
    """The stream ends one byte short of, at and past the dword of lines 63, 64, 65 and 127 of the window (line k's dword is
    the four bytes from first_line + 128 k): the second load's range with the end inside it; tile 3 at and past the end."""
    cases = []
    for in_off in (0, 1, 127, 128 * 77 + 5):
        tile3 = in_off + PROLOGUE
        line = tile3 // LINE * LINE
        for cap in CAPS:
            for past in PASTS:
                for k in (0, 1, 2, 62, 63, 64, 65, 66, 126, 127, 128):
                    for d in (3, 4, 5):
                        if line + LINE * k + d > tile3 - 4:
                            cases.append((in_off, 40000, line + LINE * k + d, cap, past))        # a unit longer than any window
                            cases.append((in_off, line + LINE * k + d - in_off, line + LINE * k + d, cap, past))  # the stream's last unit
        for enc_bytes in range(max(8, tile3 - 3), tile3 + 2 * LINE + 6):
            cases.append((in_off, 40000, enc_bytes, 128, 0))
    got = check(exe, cases)
    for (in_off, span, enc_bytes, cap, past), (line, lines) in zip(cases, got):
        if in_off + PROLOGUE >= enc_bytes:
            assert (line, lines) == (0, 0), (in_off, enc_bytes)
    by_lines = {l for _, l in got}
    assert {0, 1, 63, 64, 65, 66, 127, 128} <= by_lines
    # line 64's dword: three of its bytes inside the stream -> 64 lines, all four -> 65
    assert run(exe, "w", [(0, 40000, PROLOGUE + LINE * 64 + 3, 128, 0), (0, 40000, PROLOGUE + LINE * 64 + 4, 128, 0)]) == [(PROLOGUE, 64), (PROLOGUE, 65)]
    # a unit that begins past the stream's end (a table the device does not trust): nothing, whatever the span
    assert run(exe, "w", [(1000, 9000, 999, 128, 0), ((1 << 64) - 1, 9000, 1 << 20, 128, 0), ((1 << 64) - 1536, U32, (1 << 64) - 1, 128, 1536),
                          (0, U32, 8, 128, 0)]) == [(0, 0)] * 4


def test_offsets_around_4_gib_and_above_2_47_are_64_bit(exe):
    cases = [((1 << 32) + d, span, (1 << 32) + end, cap, past)
             for d in (-20000, -9728, -9727, -1537, -1536, -1535, -130, -1, 0, 1, 127)
             for end in (-1, 0, 1, 4, 200, 4096, 8192 + 260, 1 << 20) for span in (1537, 9000, 17000, U32) for cap in (64, 128) for past in PASTS]
    cases += [((1 << 33) - 1, 9000, 1 << 34, 128, 0), ((1 << 47) + 3, 9000, (1 << 47) + 4000, 128, 0), ((1 << 47) + 3, 17000, (1 << 48), 128, 1536),
              ((1 << 47) + 127, U32, (1 << 47) + (1 << 33), 128, 0), ((1 << 63) + 5, 17000, (1 << 64) - 1, 128, 0)]
    got = check(exe, cases)
    assert sum(1 for line, lines in got if lines and line >= 1 << 32) >= 8        # windows wholly above 2^32 ...
    assert sum(1 for line, lines in got if lines > 64 and line + 64 * LINE <= 1 << 32 < line + LINE * lines) >= 2  # ... and 2^32 inside the second load's lines
    assert sum(1 for line, lines in got if lines and line < 1 << 32 <= line + 64 * LINE) >= 2
    assert run(exe, "w", [((1 << 32) - 1536, 40000, (1 << 32) + 4096, 128, 0)]) == [(1 << 32, 32)]  # (4096 - 4) // 128 + 1


def test_spans_of_2_32_minus_1_and_saturated(exe):
    got = check(exe, [(in_off, span, enc, cap, past) for in_off in (0, 127, (1 << 32) - 5) for span in (U32 - 1, U32)
                      for enc in (BIG, in_off + 20000, in_off + U32) for cap in CAPS for past in PASTS])
    assert {l for _, l in got} == set(CAPS)  # (the streams are longer than any window: the cap binds)
    # the picker saturates: a last record 2^33 bytes before the stream's end, n so large that 6 n does not cut
    assert run(exe, "s", [(0, U32, 0, 0, 1 << 33), (5, U32, 1, 5 + (1 << 32), 1 << 40), (5, U32, 1, 5 + U32, 1 << 40), (5, U32, 1, 4 + U32, 1 << 40)]) == [U32, U32, U32, U32 - 1]


def test_the_span_picker(exe):
    cases = []
    for in_off in (0, 1000, (1 << 32) - 100, (1 << 47) + 1):
        for n in (1, 2, 256, 2589, 16384):
            for nxt in (in_off + 1, in_off + 2, in_off + 6 * n - 1, in_off + 6 * n, in_off + 6 * n + 1, in_off + 9000, in_off + (1 << 33),  # greater
                        in_off, max(in_off - 1, 0), 0):                                                                                     # equal, lower
                cases.append((in_off, n, 1, nxt, in_off + (1 << 34)))
            for enc in (in_off + 1, in_off + 2, in_off + 8611, in_off + 6 * n, in_off + 6 * n + 1, in_off, max(in_off - 1, 0)):           # absent: the last record
                cases.append((in_off, n, 0, 12345, enc))
    got = run(exe, "s", cases)
    for c, g in zip(cases, got):
        assert g == span_model(*c), (c, g)
    assert run(exe, "s", [(1000, 16384, 1, 9600, 1 << 20), (1000, 16384, 1, 1000, 1 << 20), (1000, 16384, 1, 999, 1 << 20),
                          (1000, 16384, 0, 5, 9600), (1000, 16384, 0, 5, 1000)]) == [8600, 0, 0, 8600, 0]
    # the cut: a record far ahead (a partial or scattered table) bounds nothing, 6 n does
    assert run(exe, "s", [(0, n, 1, 1 << 30, 1 << 31) for n in (1, 2589, 16384)]) == [6, 15534, 98304]


def test_an_unknown_span_falls_back_to_the_rule_of_n(exe):
    cases = [(in_off, n, 0, enc, cap, past) for in_off in (0, 1, 127, 5000, (1 << 32) - 3000) for n in (1, 2588, 2589, 3000, 8192, 16384, 1 << 28)
             for enc in (BIG, in_off + 1536, in_off + 1537, in_off + 4000, in_off + 9000) for cap in (64, 128) for past in PASTS]
    got = run(exe, "u", cases)
    for (in_off, n, _, enc, cap, past), g in zip(cases, got):
        assert g == old_model(in_off, n, enc), (in_off, n, enc, cap, past, g)  # (64 lanes at the most, whatever the cap of the span's rule)
    # ... and a known one does not
    known = [(in_off, 16384, span, BIG, 128, 0) for in_off in (0, 127) for span in (1, 1537, 6000, 17000)]
    assert run(exe, "u", known) == [model(i, s, e, c, p) for i, _, s, e, c, p in known]


# ---- the build -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_the_span_and_the_second_load_cost_no_register(tmp_path):
    spec = importlib.util.spec_from_file_location("check_inflight", os.path.join(ROOT, "tools", "check_inflight.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    res = tool.kernel_resources(tool.compile_to_asm(str(tmp_path / "shipped")))
    single = [k for k in res if "dint_dev20decode_single_kernelE" in k]
    assert len(single) == 1
    r = res[single[0]]
    assert r["vgpr_count"] <= 128 and r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["sgpr_spill_count"] <= 56, r  # what the build with the window sized from n had
