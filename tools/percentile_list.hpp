// dint_queries --percentiles LIST: the ranks of the percentile query types as text: decimal percents separated by commas,
// each digits with at most four fractional digits behind an optional point ("50", "99.9", "0.0001"), between 0 and 100, at
// most 16 of them (DINT_PERCENTILES_MAX), in any order, repeats allowed -> parts per million, without floating point: the
// integer part times 10000 plus the fraction padded to four digits. Refused: an empty list or item, a sign, a blank, an
// exponent or any other non-digit, a point without a digit on both sides, more than four fractional digits, a value above
// 100 and more than 16 entries. Plain C++, beside value_edges.hpp.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace tool {

constexpr size_t kPercentilesMost = 16;

inline std::vector<uint32_t> parse_percentiles(const std::string& text) {
    auto bad = [&](const char* why) { return std::runtime_error(std::string("--percentiles: ") + why + ": " + text); };
    std::vector<uint32_t> per_million;
    for (size_t at = 0;;) {
        const size_t comma = text.find(',', at);
        const std::string item = text.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        const size_t point = item.find('.');
        const std::string whole = item.substr(0, point);
        const std::string part = point == std::string::npos ? std::string() : item.substr(point + 1);
        if (whole.empty() || whole.find_first_not_of("0123456789") != std::string::npos || part.find_first_not_of("0123456789") != std::string::npos ||
            (point != std::string::npos && part.empty()))
            throw bad("not a comma-separated list of decimal numbers");
        if (part.size() > 4) throw bad("more than four fractional digits");
        if (whole.size() > 3) {  // (leading zeros aside, a number above 999)
            if (whole.find_first_not_of('0') < whole.size() - 3) throw bad("a percentile above 100");
        }
        uint32_t p = 0;
        for (char c : whole.size() > 3 ? whole.substr(whole.size() - 3) : whole) p = p * 10 + uint32_t(c - '0');
        uint32_t f = 0;
        for (size_t i = 0; i != 4; ++i) f = f * 10 + (i < part.size() ? uint32_t(part[i] - '0') : 0u);
        p = p * 10000 + f;
        if (p > 1000000) throw bad("a percentile above 100");
        if (per_million.size() == kPercentilesMost) throw bad("more than 16 percentiles");
        per_million.push_back(p);
        if (comma == std::string::npos) return per_million;
        at = comma + 1;
    }
}

}  // namespace tool
