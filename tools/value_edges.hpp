// dint_queries --edges LIST: the bucket boundaries of the value-stats query types as text: decimal u32 values separated by
// commas, strictly ascending, at most 1023 of them (DINT_VALUE_STATS_MAX_EDGES). Refused: an empty list or item, a sign, a
// blank, hex or any other non-digit, a value above 2^32 - 1, more than 1023 edges and a list that is not strictly ascending.
// Plain C++, beside doc_values_file.hpp.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace tool {

constexpr size_t kValueEdgesMost = 1023;

inline std::vector<uint32_t> parse_value_edges(const std::string& text) {
    auto bad = [&](const char* why) { return std::runtime_error(std::string("--edges: ") + why + ": " + text); };
    std::vector<uint32_t> edges;
    for (size_t at = 0;;) {
        const size_t comma = text.find(',', at);
        const std::string digits = text.substr(at, comma == std::string::npos ? std::string::npos : comma - at);
        if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos) throw bad("not a comma-separated list of decimal numbers");
        if (digits.size() > 10 || std::stoull(digits) > 0xFFFFFFFFull) throw bad("an edge above 4294967295");
        const uint32_t e = uint32_t(std::stoull(digits));
        if (!edges.empty() && edges.back() >= e) throw bad("the edges are not strictly ascending");
        if (edges.size() == kValueEdgesMost) throw bad("more than 1023 edges");
        edges.push_back(e);
        if (comma == std::string::npos) return edges;
        at = comma + 1;
    }
}

}  // namespace tool
