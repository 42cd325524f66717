// tests/test_stream_touch_span_cpu.py: the window of a unit whose byte span is known, and the span picker (dint_stream_touch.hpp),
// compiled alone. stdin: one case per line,
//   "w in_off span enc_bytes max_lines past"        -> "first_line lines"   stream_touch_span
//   "s in_off n has_next next_in_off enc_bytes"      -> "span"               unit_stream_span
//   "u in_off n span enc_bytes max_lines past"       -> "first_line lines"   unit_touch (span 0: the rule of n)
#include <cinttypes>
#include <cstdio>

#include "dint_stream_touch.hpp"

// (usable in constant expressions: what the header promises host and device code alike)
static_assert(dint_dev::stream_touch_span(0, 1536 + 8192, 1u << 20, 128, 0).lines == 64, "8 KB behind tile 2 from a line's first byte: 64 lines");
static_assert(dint_dev::stream_touch_span(0, 1536 + 8193, 1u << 20, 128, 0).lines == 65, "one byte more: the second load");
static_assert(dint_dev::stream_touch_span(0, 1536, 1u << 20, 128, 0).lines == 0, "the prologue's three tiles cover the unit");
static_assert(dint_dev::unit_stream_span(100, 16384, true, 9000, 1u << 20) == 8900, "up to the next record");
static_assert(dint_dev::unit_stream_span(100, 16384, true, 100, 1u << 20) == 0, "a record twice: not known");
static_assert(dint_dev::unit_touch(0, 16384, 0, 1u << 20, 128, 0).lines == dint_dev::stream_touch(0, 16384, 1u << 20).lanes, "the fallback");

int main() {
    char what;
    while (std::scanf(" %c", &what) == 1) {
        if (what == 'w' || what == 'u') {
            uint64_t in_off, enc_bytes;
            uint32_t a, b, max_lines, past;  // w: span; u: n, span
            if (what == 'w') {
                if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &in_off, &a, &enc_bytes, &max_lines, &past) != 5) return 1;
                const dint_dev::stream_touch_lines w = dint_dev::stream_touch_span(in_off, a, enc_bytes, max_lines, past);
                std::printf("%" PRIu64 " %" PRIu32 "\n", w.first_line, w.lines);
            } else {
                if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu32 " %" SCNu32, &in_off, &a, &b, &enc_bytes, &max_lines, &past) != 6) return 1;
                const dint_dev::stream_touch_lines w = dint_dev::unit_touch(in_off, a, b, enc_bytes, max_lines, past);
                std::printf("%" PRIu64 " %" PRIu32 "\n", w.first_line, w.lines);
            }
        } else if (what == 's') {
            uint64_t in_off, next_in_off, enc_bytes;
            uint32_t n, has_next;
            if (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64, &in_off, &n, &has_next, &next_in_off, &enc_bytes) != 5) return 1;
            std::printf("%" PRIu32 "\n", dint_dev::unit_stream_span(in_off, n, has_next != 0, next_in_off, enc_bytes));
        } else {
            return 1;
        }
    }
    return 0;
}
