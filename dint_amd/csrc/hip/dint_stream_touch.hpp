// The stream touch of the vroom single-dictionary segments (kernels/segment.inc, TOUCH): which 128-byte lines of the
// compressed stream a wave asks for — one dword a lane, its value used for nothing — in the same trip to memory as its
// unit's first three tiles, so that the unit's later slot requests find their lines in L2. Plain C++: host code (the
// rules' own tests, tests/cpp/stream_touch_cases.cpp and tests/cpp/stream_touch_span_cases.cpp) and device code include this file.
#pragma once
#include <stdint.h>

// Lanes of the touch at the most (a lane = one 128-byte line): 0 = no touch, the loop as it was (the A/B baseline);
// 64 = 8 KB, what a 16384-integer unit has left behind its third tile. Measured at 10^9 postings against the loop without
// (profiles/r08_ab_stream_touch.txt): 16 lanes -0.0 to -0.5 %, 32 lanes -2.1 to -2.9 %, 64 lanes -5.0 to -7.5 %.
#ifndef DINT_STREAM_TOUCH_LANES
#define DINT_STREAM_TOUCH_LANES 64
#endif
static_assert(DINT_STREAM_TOUCH_LANES >= 0 && DINT_STREAM_TOUCH_LANES <= 64, "DINT_STREAM_TOUCH_LANES: 0 to 64");
// Lines of a unit's window at the most where the unit's byte span is known (stream_touch_span below): 0 to 128 — two loads of
// DINT_STREAM_TOUCH_LANES lanes, the second under a wave-uniform `lines > 64`. DINT_STREAM_TOUCH_LANES stays the lanes of ONE
// load, and 0 there still compiles every touch out.
#ifndef DINT_STREAM_TOUCH_LINES
#define DINT_STREAM_TOUCH_LINES 128
#endif
static_assert(DINT_STREAM_TOUCH_LINES >= 0 && DINT_STREAM_TOUCH_LINES <= 128, "DINT_STREAM_TOUCH_LINES: 0 to 128");
// Bytes past the unit's last one that the window of a known span covers as well: 1536 = the next unit's first three tiles —
// what the wave that draws the next ticket of the shard asks for in ITS prologue's trip, a fraction of a microsecond later,
// and then finds in L2 or on its way. With it, every byte of a run of long units is touched ahead by the unit before. Measured at
// 10^9 postings against the window sized from n (profiles/r09_ab_touch_span.txt; one box, three processes): 0 past -1.3 to
// -1.8 %, 512 -2.2 to -2.3 %, 1024 -2.2 to -2.6 %, 1536 -2.7 to -2.8 %, 2048 -2.9 to -3.3 %, 3072 -3.0 to -3.1 %.
#ifndef DINT_STREAM_TOUCH_PAST
#define DINT_STREAM_TOUCH_PAST 1536
#endif
static_assert(DINT_STREAM_TOUCH_PAST >= 0 && DINT_STREAM_TOUCH_PAST <= 16384, "DINT_STREAM_TOUCH_PAST: 0 to 16384 bytes");

namespace dint_dev {

constexpr uint32_t kTouchLineBytes = 128;
constexpr uint32_t kTouchPrologueBytes = 3 * 512;  // tiles 0, 1 and 2 of 256 16-bit slots: what the prologue asks for itself
// A vroom unit's byte span is not in the unit table: n integers are taken for n * 19 / 32 stream bytes — the bench stream's
// 0.564 bytes an integer and a twentieth more, which is 8 KB (64 lines) behind the third tile of a unit of 16384. A unit that
// is shorter than that touches the first bytes of the next one, which a wave of the same queue shard reads next; a longer one
// finds its last lines in HBM as before.
constexpr uint32_t kTouchBytesPer32Ints = 19;
constexpr uint32_t kTouchMaxInts = 1u << 20;  // (more integers than any cap needs: the arithmetic on n stays 32-bit)

struct stream_touch_window {
    uint64_t first_line;  // byte offset of the first line touched (a multiple of 128, below enc_bytes); 0 where lanes == 0
    uint32_t lanes;       // lane l < lanes reads the dword at first_line + 128 l, every byte of it below enc_bytes
};

// in_off: the unit's first stream byte; n: its integers; enc_bytes: the stream's length.
constexpr stream_touch_window stream_touch(uint64_t in_off, uint32_t n, uint64_t enc_bytes,
                                           uint32_t max_lanes = DINT_STREAM_TOUCH_LANES) {
    // tile 3's first byte at or past the stream's end: nothing to touch (in_off itself may be anything)
    if (in_off > enc_bytes || enc_bytes - in_off <= kTouchPrologueBytes) return {0, 0};
    const uint32_t bytes = (n < kTouchMaxInts ? n : kTouchMaxInts) * kTouchBytesPer32Ints / 32;
    if (bytes <= kTouchPrologueBytes) return {0, 0};  // the prologue's three tiles cover the unit
    const uint64_t tile3 = in_off + kTouchPrologueBytes;
    const uint64_t line = tile3 & ~uint64_t(kTouchLineBytes - 1);
    // lines from `line` on that hold the unit's bytes behind tile 2 ...
    const uint32_t want = (uint32_t(tile3 - line) + (bytes - kTouchPrologueBytes) + kTouchLineBytes - 1) / kTouchLineBytes;
    uint32_t lanes = want < max_lanes ? want : max_lanes;
    // ... and whose first dword lies inside the stream (line <= tile3 < enc_bytes: room is at least 1)
    const uint32_t room = enc_bytes - line < 0xFFFFFFFFull ? uint32_t(enc_bytes - line) : 0xFFFFFFFFu;  // (saturated: 64 lanes are 8 KB)
    if (room < 4) return {0, 0};
    const uint32_t fit = (room - 4) / kTouchLineBytes + 1;
    if (fit < lanes) lanes = fit;
    if (lanes == 0) return {0, 0};
    return {line, lanes};
}

// ---- the window of a unit whose byte span is known -----------------------------------------------------------------------
// The rule above fits the bench's own stream badly (tools/touch_window_model.py, profiles/r09_touch_window_model.txt): a unit of
// 16384 integers spans 5.1 to 17 KB there, dense lists and sparse ones a factor of three apart. A third of the long units reach
// past a window sized from n, and a fifth of the stream is touched behind the end of the unit that touches it. Where a unit's span
// IS known — the next record of the table begins where this one ends — the window is the unit's own lines and nothing else.
struct stream_touch_lines {
    uint64_t first_line;  // byte offset of the first line touched (a multiple of 128, below enc_bytes); 0 where lines == 0
    uint32_t lines;       // line l < lines is touched by the dword at first_line + 128 l, every byte of it below enc_bytes
};

// in_off: the unit's first stream byte; span_bytes: its stream bytes; enc_bytes: the stream's length. The lines from the one
// that holds tile 3's first byte through the one that holds the byte `past` behind the unit's last; none for a unit that the
// prologue's three tiles cover; at most max_lines.
constexpr stream_touch_lines stream_touch_span(uint64_t in_off, uint32_t span_bytes, uint64_t enc_bytes,
                                               uint32_t max_lines = DINT_STREAM_TOUCH_LINES, uint32_t past = DINT_STREAM_TOUCH_PAST) {
    if (in_off > enc_bytes || enc_bytes - in_off <= kTouchPrologueBytes) return {0, 0};
    if (span_bytes <= kTouchPrologueBytes) return {0, 0};
    const uint64_t tile3 = in_off + kTouchPrologueBytes;
    const uint64_t line = tile3 & ~uint64_t(kTouchLineBytes - 1);
    // (64-bit: a span of 2^32 - 1 and `past` on top of it)
    const uint64_t want = (uint64_t(tile3 - line) + (uint64_t(span_bytes) - kTouchPrologueBytes) + past + kTouchLineBytes - 1) / kTouchLineBytes;
    uint32_t lines = want < max_lines ? uint32_t(want) : max_lines;
    const uint32_t room = enc_bytes - line < 0xFFFFFFFFull ? uint32_t(enc_bytes - line) : 0xFFFFFFFFu;  // (saturated: 128 lines are 16 KB)
    if (room < 4) return {0, 0};
    const uint32_t fit = (room - 4) / kTouchLineBytes + 1;
    if (fit < lines) lines = fit;
    if (lines == 0) return {0, 0};
    return {line, lines};
}

// A unit's byte span from the unit table, as bundle_schedule_kernel bounds it: up to the next record's first byte, for the
// table's last record up to the stream's end; 0 = not known — the next record begins at or before this one (a table in another
// order than the stream's, a record twice), or this one begins at or past the stream's end. Between two records of a partial or
// scattered table lie units that the table leaves out: the span is cut to 6 n bytes — a 16-bit slot decodes to at least one integer
// and the longest codeword of one integer is a 32-bit exception, 2 + 4 bytes — and saturated to 32 bits.
constexpr uint32_t unit_stream_span(uint64_t in_off, uint32_t n, bool has_next, uint64_t next_in_off, uint64_t enc_bytes) {
    const uint64_t end = has_next ? next_in_off : enc_bytes;
    if (end <= in_off) return 0;
    const uint64_t longest = 6ull * n;
    const uint64_t span = end - in_off < longest ? end - in_off : longest;
    return span < 0xFFFFFFFFull ? uint32_t(span) : 0xFFFFFFFFu;
}

// The window of a unit: its own lines where its span is known (span_bytes != 0), the rule of n where it is not.
constexpr stream_touch_lines unit_touch(uint64_t in_off, uint32_t n, uint32_t span_bytes, uint64_t enc_bytes,
                                        uint32_t max_lines = DINT_STREAM_TOUCH_LINES, uint32_t past = DINT_STREAM_TOUCH_PAST) {
    if (span_bytes != 0) return stream_touch_span(in_off, span_bytes, enc_bytes, max_lines, past);
    const stream_touch_window w = stream_touch(in_off, n, enc_bytes);
    return {w.first_line, w.lanes};
}

}  // namespace dint_dev
