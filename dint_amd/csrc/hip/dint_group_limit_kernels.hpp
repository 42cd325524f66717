// Group-limited ranked queries: of every document group a query matches, up to per_group documents reach the selection
// (DESIGN.md 4d-group-limit). A top-n per group is a selection, not a maximum, but it is an ITERATED bounded maximum: the
// group's place r is the largest key strictly below its place r - 1. The table is top[q][r][g] — query-major, then place,
// then group — so a place's row is n_groups contiguous 64-bit words, what collapse_max expects of best_row; a zero entry
// means "no such match" (a live key is never 0). group_limit_round_kernel runs once per place, in stream order, with nothing
// on the host between the launches; group_limit_keep_kernel kills every grouped slot below its group's last place and counts
// the survivors; behind the selection group_limit_hits_kernel names every hit's group, that group's matches and the hit's
// place in it. Every step is a 64-bit maximum or an integer add: the answer is exact and the same from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_collapse_kernels.hpp"

namespace dint_dev {

// Place r of every (query, group) of a ranked call's slots: a workgroup of 256 per page, a thread per slot, as the other slot
// kernels. page_query[page] + q0 is the page's query of the call, top + (that * per_group + r) * n_groups the row of its
// place r (zero where no key has arrived).
//  - r == 0 is collapse_best_kernel's job: a dead slot and a match in no group (kFacetNone in the map, or at or past its
//    num_docs) carry kFacetNone, slot_group[i] <- the slot's group, and the maximum goes into row (q, 0).
//  - r >= 1 reads slot_group and does not gather the map again. A live grouped slot offers its key iff it is strictly below
//    its group's place r - 1; a group whose place r - 1 is empty has bound 0, and nothing of it offers. Every other lane
//    carries kFacetNone, which breaks runs and offers nothing.
// Every thread reaches collapse_max: its barriers, its DPP moves and its ballot. No word past n_slots is read.
__global__ __launch_bounds__(256) void group_limit_round_kernel(const uint32_t* cand, const float* score, uint64_t n_slots,
                                                                const uint32_t* page_query, uint32_t q0, doc_facets_view f, uint32_t r,
                                                                uint32_t per_group, unsigned long long* top, uint32_t* slot_group) {
    __shared__ unsigned long long bins[kFacetBins];
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    unsigned long long* const row = top + (uint64_t(page_query[blockIdx.x] + q0) * per_group + r) * f.n_groups;
    uint32_t g = kFacetNone;
    unsigned long long key = 0ull;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (r == 0) {  // (uniform)
            if (d != kDeadCandidate) {
                g = facet_group(f, d);
                if (g != kFacetNone) key = collapse_key(score[i], d);
            }
            slot_group[i] = g;
        } else if (d != kDeadCandidate) {
            const uint32_t sg = slot_group[i];
            if (sg != kFacetNone) {
                const unsigned long long mine = collapse_key(score[i], d);
                if (mine < (row - f.n_groups)[sg]) g = sg, key = mine;  // (the row of place r - 1)
            }
        }
    }
    collapse_max(g, key, f.n_groups, bins, row);
}

// A live slot in a group whose key is below the group's place per_group - 1 dies. An empty last place (0) means the group
// has fewer than per_group matches: no key is below it, and all of them stay. Keys are unique within a query (docIDs are), so
// exactly min(per_group, matches) slots per matched group survive. The survivors — the ungrouped matches among them, which
// stand for themselves — are counted into kept[the page's query]: a ballot and at most one add per wave.
__global__ __launch_bounds__(256) void group_limit_keep_kernel(uint32_t* cand, const float* score, const uint32_t* slot_group, uint64_t n_slots,
                                                               const uint32_t* page_query, uint32_t q0, uint32_t n_groups, uint32_t per_group,
                                                               const unsigned long long* top, unsigned long long* kept) {
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    const uint32_t q = page_query[blockIdx.x] + q0;
    bool keep = false;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate) {
            const uint32_t g = slot_group[i];
            keep = g == kFacetNone || collapse_key(score[i], d) >= top[(uint64_t(q) * per_group + (per_group - 1u)) * n_groups + g];
            if (!keep) cand[i] = kDeadCandidate;
        }
    }
    const unsigned long long keeps = __ballot(keep);
    if ((threadIdx.x & 63u) == 0 && keeps) atomicAdd(&kept[q], static_cast<unsigned long long>(__popcll(keeps)));
}

// Behind the selection, a thread per (query of the pass, i): keys[q * k + i] is the query's i-th best key (0 past its
// count). hit_groups / hit_group_matches at (q0 + q) * k + i as collapse_hits_kernel writes them; hit_group_ranks there <-
// the place r with top[q][r][g] == key, the hit's 0-based position among all matches of its group in key order (a kept
// grouped hit holds one of its group's places; 0 for an ungrouped hit and past the count).
__global__ void group_limit_hits_kernel(const unsigned long long* keys, uint32_t n_queries, uint32_t k, uint32_t q0, doc_facets_view f,
                                        uint32_t per_group, const uint32_t* rows, const unsigned long long* top, uint32_t* hit_groups,
                                        uint32_t* hit_group_matches, uint32_t* hit_group_ranks) {
    const uint64_t x = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= uint64_t(n_queries) * k) return;
    const uint64_t q = q0 + x / k;
    const unsigned long long key = keys[x];
    uint32_t g = kFacetNone, n = 0, rank = 0;
    if (key) {
        g = facet_group(f, 0xFFFFFFFFu - uint32_t(key));
        n = g == kFacetNone ? 1u : rows[q * f.n_groups + g];
        if (g != kFacetNone)
            for (uint32_t r = 1; r < per_group; ++r)
                if (top[(q * per_group + r) * f.n_groups + g] == key) rank = r;
    }
    hit_groups[q * k + x % k] = g;
    hit_group_matches[q * k + x % k] = n;
    hit_group_ranks[q * k + x % k] = rank;
}

}  // namespace dint_dev
