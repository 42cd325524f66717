// dint_queries --facets FILE: a document -> group map as text. Every line is `d g` (document d is in group g) or `lo:hi g`
// (every document of the half-open interval [lo, hi) is). Later lines win over earlier ones; a document no line names is in
// no group. Blank lines and an empty interval (lo >= hi) are legal. DocIDs are below 0xFFFFFFFF, so d <= 0xFFFFFFFE and
// hi <= 0xFFFFFFFF; groups are below 65536 (DINT_FACETS_MAX_GROUPS). Plain C++ over <istream>: tests/test_facets_cpu.py
// compiles this file alone.
#pragma once
#include <cstdint>
#include <istream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace tool {

// A map as dint_doc_facets_create takes it: num_docs = the largest docID a line names + 1 (0: no document is in a group),
// group_of[d] the group or 0xFFFFFFFF (DINT_FACET_NONE), n_groups = the largest group a line names + 1 (at least 1).
struct doc_facets_map {
    std::vector<uint32_t> group_of;
    uint64_t num_docs = 0;
    uint32_t n_groups = 1;
};

inline doc_facets_map parse_doc_facets(std::istream& in) {
    auto number = [](const std::string& digits, const std::string& line, uint64_t most) {
        if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 || std::stoull(digits) > most)
            throw std::runtime_error("--facets: not a `d g` or `lo:hi g` line: " + line);
        return uint64_t(std::stoull(digits));
    };
    struct run {
        uint64_t lo, hi;  // [lo, hi), not empty
        uint32_t g;
    };
    std::vector<run> runs;
    doc_facets_map f;
    for (std::string line; std::getline(in, line);) {
        std::istringstream words(line);
        std::string docs, group, more;
        if (!(words >> docs)) continue;
        if (!(words >> group) || (words >> more)) throw std::runtime_error("--facets: not a `d g` or `lo:hi g` line: " + line);
        const uint32_t g = uint32_t(number(group, line, 65535));
        if (g + 1 > f.n_groups) f.n_groups = g + 1;  // (an empty interval's group is a group too: its row is zeros)
        const size_t colon = docs.find(':');
        uint64_t lo, hi;
        if (colon == std::string::npos) {
            lo = number(docs, line, 0xFFFFFFFEull);
            hi = lo + 1;
        } else {
            lo = number(docs.substr(0, colon), line, 0xFFFFFFFFull);
            hi = number(docs.substr(colon + 1), line, 0xFFFFFFFFull);
        }
        if (lo >= hi) continue;
        runs.push_back({lo, hi, g});
        if (hi > f.num_docs) f.num_docs = hi;
    }
    f.group_of.assign(f.num_docs, 0xFFFFFFFFu);
    for (auto const& r : runs)  // (in the file's order: later lines win)
        for (uint64_t d = r.lo; d != r.hi; ++d) f.group_of[d] = r.g;
    return f;
}

}  // namespace tool
