// dint_queries --filter FILE: a document filter as text. Every line is a docID `d` or a half-open interval `lo:hi`; the
// filter is the union of the lines. Blank lines, an empty interval (lo >= hi) and overlapping lines are legal. DocIDs are
// below 0xFFFFFFFF, so d <= 0xFFFFFFFE and hi <= 0xFFFFFFFF. Plain C++ over <istream>: tests/test_doc_filter_cpu.py compiles
// this file alone.
#pragma once
#include <cstdint>
#include <istream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace tool {

// A filter as dint_doc_filter_create takes it: num_docs = the largest docID of the filter + 1 (0: the empty filter),
// ceil(num_docs / 64) words.
struct doc_filter_bits {
    std::vector<uint64_t> words;
    uint64_t num_docs = 0;
};

inline doc_filter_bits parse_doc_filter(std::istream& in) {
    auto number = [](const std::string& digits, const std::string& line) {
        if (digits.empty() || digits.find_first_not_of("0123456789") != std::string::npos || digits.size() > 10 ||
            std::stoull(digits) > 0xFFFFFFFFull)
            throw std::runtime_error("--filter: not a docID or a lo:hi interval: " + line);
        return uint64_t(std::stoull(digits));
    };
    std::vector<std::pair<uint64_t, uint64_t>> runs;  // [lo, hi), not empty
    doc_filter_bits f;
    for (std::string line; std::getline(in, line);) {
        const size_t a = line.find_first_not_of(" \t\r"), b = line.find_last_not_of(" \t\r");
        if (a == std::string::npos) continue;
        const std::string tok = line.substr(a, b - a + 1);
        const size_t colon = tok.find(':');
        uint64_t lo, hi;
        if (colon == std::string::npos) {
            lo = number(tok, tok);
            if (lo == 0xFFFFFFFFull) throw std::runtime_error("--filter: not a docID or a lo:hi interval: " + tok);
            hi = lo + 1;
        } else {
            lo = number(tok.substr(0, colon), tok);
            hi = number(tok.substr(colon + 1), tok);
        }
        if (lo >= hi) continue;
        runs.emplace_back(lo, hi);
        if (hi > f.num_docs) f.num_docs = hi;
    }
    f.words.assign((f.num_docs + 63) / 64, 0ull);
    for (auto const& r : runs) {
        const uint64_t w0 = r.first >> 6, w1 = (r.second - 1) >> 6;  // the words of the first and the last docID
        const uint64_t from = ~0ull << (r.first & 63), upto = ~0ull >> (63 - ((r.second - 1) & 63));
        if (w0 == w1) {
            f.words[w0] |= from & upto;
            continue;
        }
        f.words[w0] |= from;
        for (uint64_t w = w0 + 1; w != w1; ++w) f.words[w] = ~0ull;
        f.words[w1] |= upto;
    }
    return f;
}

}  // namespace tool
