// dint_queries --values FILE: a document -> u32 value column as text. Every line is `d v` (document d has value v) or
// `lo:hi v` (every document of the half-open interval [lo, hi) has). Later lines win over earlier ones; a document no line
// names has value 0. Blank lines and an empty interval (lo >= hi) are legal. DocIDs are below 0xFFFFFFFF, so d <= 0xFFFFFFFE
// and hi <= 0xFFFFFFFF; every u32 is a value. Plain C++ over <istream>, beside doc_facets_file.hpp.
#pragma once
#include <cstdint>
#include <istream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace tool {

// A column as dint_doc_values_create takes it: num_docs = the largest docID a line names + 1 (0: an empty column).
struct doc_values_column {
    std::vector<uint32_t> values;
    uint64_t num_docs = 0;
};

// `lo:hi` of --value-range: the closed interval of values [lo, hi]
inline void parse_value_range(const std::string& text, uint32_t& lo, uint32_t& hi) {
    auto number = [&](const std::string& digits) {
        if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 ||
            std::stoull(digits) > 0xFFFFFFFFull)
            throw std::runtime_error("--value-range: not lo:hi: " + text);
        return uint32_t(std::stoull(digits));
    };
    const size_t colon = text.find(':');
    if (colon == std::string::npos) throw std::runtime_error("--value-range: not lo:hi: " + text);
    lo = number(text.substr(0, colon));
    hi = number(text.substr(colon + 1));
}

inline doc_values_column parse_doc_values(std::istream& in) {
    auto number = [](const std::string& digits, const std::string& line, uint64_t most) {
        if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 || std::stoull(digits) > most)
            throw std::runtime_error("--values: not a `d v` or `lo:hi v` line: " + line);
        return uint64_t(std::stoull(digits));
    };
    struct run {
        uint64_t lo, hi;  // [lo, hi), not empty
        uint32_t v;
    };
    std::vector<run> runs;
    doc_values_column c;
    for (std::string line; std::getline(in, line);) {
        std::istringstream words(line);
        std::string docs, value, more;
        if (!(words >> docs)) continue;
        if (!(words >> value) || (words >> more)) throw std::runtime_error("--values: not a `d v` or `lo:hi v` line: " + line);
        const uint32_t v = uint32_t(number(value, line, 0xFFFFFFFFull));
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
        runs.push_back({lo, hi, v});
        if (hi > c.num_docs) c.num_docs = hi;
    }
    c.values.assign(c.num_docs, 0u);
    for (auto const& r : runs)  // (in the file's order: later lines win)
        for (uint64_t d = r.lo; d != r.hi; ++d) c.values[d] = r.v;
    return c;
}

}  // namespace tool
