// tests/test_stream_touch_cpu.py: the window rule of the single-dictionary segments' stream touch (dint_stream_touch.hpp),
// compiled alone. stdin: one case per line, "in_off n enc_bytes max_lanes"; stdout: "first_line lanes" per case.
#include <cinttypes>
#include <cstdio>

#include "dint_stream_touch.hpp"

// (the rule is usable in constant expressions: what the header promises host and device code alike)
static_assert(dint_dev::stream_touch(0, 16384, 1u << 20, 64).lanes == 64, "a unit of 16384 integers takes the full cap");
static_assert(dint_dev::stream_touch(0, 16384, 1u << 20, 64).first_line == 1536, "tile 3 of a unit at offset 0");
static_assert(dint_dev::stream_touch(0, 16384, 8, 64).lanes == 0, "the smallest stream");

int main() {
    uint64_t in_off, enc_bytes;
    uint32_t n, max_lanes;
    while (std::scanf("%" SCNu64 " %" SCNu32 " %" SCNu64 " %" SCNu32, &in_off, &n, &enc_bytes, &max_lanes) == 4) {
        const dint_dev::stream_touch_window w = dint_dev::stream_touch(in_off, n, enc_bytes, max_lanes);
        std::printf("%" PRIu64 " %" PRIu32 "\n", w.first_line, w.lanes);
    }
    return 0;
}
