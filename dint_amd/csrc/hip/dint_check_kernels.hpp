// An index checked against its collection (the reference's verify_collection, include/ds2i/verify_collection.hpp:7-52):
// DESIGN.md 4d-check.
//
// The host decodes the index pass by pass into pages (docs and freqs, 256 slots per block: dint_index_max_weights' passes)
// and streams the collection's postings of the same blocks in beside them; check_pages_kernel compares a page with what
// the collection holds there. Two results leave it, both a function of (index, collection) alone: how many postings
// differ — a sum, which no order of additions changes — and the smallest global ordinal of one that does — a minimum,
// which no order changes either. The block table lists the lists in order and a list's blocks in order, so the ordinal
// orders postings by (list, position): the smallest is the posting the reference's walk would have stopped at.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_kernels.hpp"
#include "dint_query_kernels.hpp"

namespace dint_dev {

// One page of a pass as the host staged it: the block's postings are words [at, at + n) of the pass's expected docIDs
// (and freqs); n == 0: a block of a list of wrong length, nothing of it is compared.
struct check_page {
    uint64_t ordinal;  // of the block's first posting among all postings of the index
    uint32_t at;
    uint32_t n;
};

constexpr unsigned long long kNoMismatch = ~0ull;

// A workgroup per page of the pass, a thread per slot. out[0] += the postings of the page whose docID or freq differs
// (one count per posting), out[1] = min(out[1], the ordinal of the first of them): one atomic each per workgroup, and
// none from a workgroup that found nothing — a faithful index issues no atomic at all. want_freqs null: docIDs only.
__global__ __launch_bounds__(256) void check_pages_kernel(const check_page* pages, const uint32_t* docs, const uint32_t* freqs,
                                                          const uint32_t* want_docs, const uint32_t* want_freqs,
                                                          unsigned long long* out) {
    __shared__ uint32_t s_count[kPageSlots / kWave];
    __shared__ uint32_t s_first[kPageSlots / kWave];
    const uint32_t page = blockIdx.x, slot = threadIdx.x;
    const check_page p = pages[page];
    bool bad = false;
    if (slot < p.n) {
        const uint64_t at = uint64_t(page) * kPageSlots + slot;
        bad = docs[at] != want_docs[p.at + slot];
        if (want_freqs) bad = bad || freqs[at] != want_freqs[p.at + slot];
    }
    const uint64_t wrong = __ballot(bad);  // (the wave's slots in lane order: the lowest set bit is its first)
    if ((slot & (kWave - 1)) == 0) {
        s_count[slot / kWave] = uint32_t(__popcll(wrong));
        s_first[slot / kWave] = wrong ? slot + uint32_t(__ffsll((long long)wrong) - 1) : kPageSlots;
    }
    __syncthreads();
    if (slot != 0) return;
    uint32_t count = 0, first = kPageSlots;
    for (uint32_t w = 0; w != kPageSlots / kWave; ++w) {
        count += s_count[w];
        first = s_first[w] < first ? s_first[w] : first;
    }
    if (count == 0) return;
    atomicAdd(&out[0], (unsigned long long)count);
    atomicMin(&out[1], (unsigned long long)(p.ordinal + first));
}

}  // namespace dint_dev
