// The stream touch of the vroom single-dictionary segments (kernels/segment.inc, TOUCH): which 128-byte lines of the
// compressed stream a wave asks for — one dword a lane, its value used for nothing — in the same trip to memory as its
// unit's first three tiles, so that the unit's later slot requests find their lines in L2. Plain C++: host code (the
// rule's own test, tests/cpp/stream_touch_cases.cpp) and device code include this file.
#pragma once
#include <stdint.h>

// Lanes of the touch at the most (a lane = one 128-byte line): 0 = no touch, the loop as it was (the A/B baseline);
// 64 = 8 KB, what a 16384-integer unit has left behind its third tile. Measured at 10^9 postings against the loop without
// (profiles/r08_ab_stream_touch.txt): 16 lanes -0.0 to -0.5 %, 32 lanes -2.1 to -2.9 %, 64 lanes -5.0 to -7.5 %.
#ifndef DINT_STREAM_TOUCH_LANES
#define DINT_STREAM_TOUCH_LANES 64
#endif
static_assert(DINT_STREAM_TOUCH_LANES >= 0 && DINT_STREAM_TOUCH_LANES <= 64, "DINT_STREAM_TOUCH_LANES: 0 to 64");

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

}  // namespace dint_dev
