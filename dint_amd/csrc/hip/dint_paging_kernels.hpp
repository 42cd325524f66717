// search_after paging of the ranked queries: the hits behind a cursor. A ranked call holds its match
// set on the device — the live slots of `cand` with their scores in front of ranked_topk — and the selection orders them by
// collapse_key (score bits, then the inverted docID), descending. A cursor is a key of that order: what lies AFTER it is
// every match whose key is strictly below. page_after_kernel kills the others in front of the selection and counts them, so
// ranked_topk, unedited, returns the best k of the rest. The comparison is on the key's bits: no tolerance, and the same
// cut from run to run; the count is an integer sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_collapse_kernels.hpp"

namespace dint_dev {

// the cursor key of a query that is read from the start: every live key is below it (its high word is no score's bits)
constexpr unsigned long long kPageFromStart = ~0ull;

// A workgroup per page, a thread per slot, as the other slot kernels. page_query[page] + q0 is the page's query of the call,
// after_key[that] its cursor key (the host's: hip_api_paging.inc). kPageFromStart: the workgroup returns — a uniform branch,
// an un-paged query pays one load. Otherwise a live slot whose key is at or above the cursor's dies, and the dead are
// counted into skipped[the page's query]: a ballot and at most one add per wave, a page belongs to one query.
__global__ __launch_bounds__(256) void page_after_kernel(uint32_t* cand, const float* score, uint64_t n_slots, const uint32_t* page_query,
                                                         uint32_t q0, const unsigned long long* after_key, unsigned long long* skipped) {
    const uint32_t q = page_query[blockIdx.x] + q0;
    const unsigned long long after = after_key[q];
    if (after == kPageFromStart) return;  // (uniform)
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    bool killed = false;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate) {
            killed = collapse_key(score[i], d) >= after;
            if (killed) cand[i] = kDeadCandidate;
        }
    }
    const unsigned long long kills = __ballot(killed);
    if ((threadIdx.x & 63u) == 0 && kills) atomicAdd(&skipped[q], static_cast<unsigned long long>(__popcll(kills)));
}

}  // namespace dint_dev
