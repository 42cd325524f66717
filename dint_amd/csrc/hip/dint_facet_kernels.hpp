// Facet counts of the ranked queries: per query, how many of its matches each document group holds.
// A facets handle maps docID -> group (a word per document, kFacetNone: in no group). A ranked call already holds its match
// set on the device — the live slots of `cand` behind the OR score kernel, behind the AND rounds — and facet_count_kernel
// reads those slots once more and scatters a count per (query, group).
// The scatter is the hot path: a few counters a query, hit by every match. What shares a destination is summed on chip
// before it touches memory (facet_add): docIDs ascend within a page and group maps are mostly clustered in docID order, so
// neighbouring lanes mostly share a group — a RUN of equal groups within a wave adds once, its length — and with at most
// kFacetBins groups the workgroup's 256 slots meet in an LDS histogram first, so a page costs at most one global add per
// group present. The handle's group sizes (the whole collection's histogram) are counted by the same function.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_ranked_or_query_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kFacetNone = 0xFFFFFFFFu;  // DINT_FACET_NONE: a document in no group
constexpr uint32_t kFacetBins = 256;          // the LDS form: a bin per thread of the workgroup

// A facets handle as the kernels see it.
struct doc_facets_view {
    const uint32_t* group_of;  // num_docs words, each below n_groups or kFacetNone (checked when the handle is made)
    uint32_t num_docs;
    uint32_t n_groups;
};
// d's group. The bound first: no word past the map is read.
__device__ __forceinline__ uint32_t facet_group(const doc_facets_view& f, uint32_t d) { return d < f.num_docs ? f.group_of[d] : kFacetNone; }

// row[g] += the threads of the workgroup whose group is g, for every g != kFacetNone. EVERY thread of a 256-thread
// workgroup calls it, with the workgroup's n_groups and row (the DPP move reads every lane, and the LDS form has
// barriers); a thread with nothing to count carries kFacetNone. g < n_groups or g == kFacetNone. bins: kFacetBins words of LDS.
//  - runs: a lane is the head of a run iff it is lane 0 or its g differs from the lane below's (lane 0 is a head whatever
//    from_lane_below gave it: that is 0, and group 0 is a group); the ballot of the heads gives a head its run's length, the
//    distance to the next head above it or to the wave's end (lane 63 has no lane above: a shift by 64 is not taken).
//    Only the heads add, and they add the length. Runs end with their wave.
//  - n_groups <= kFacetBins: the heads add to the workgroup's LDS histogram, and then thread t adds bin t to row[t] if it
//    is not zero: at most one global add per group present in the workgroup.
//  - more groups: the heads add to the row itself, one global add per run.
// Integer adds: the result is exact whatever the order.
__device__ __forceinline__ void facet_add(uint32_t g, uint32_t n_groups, uint32_t* bins, uint32_t* row) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t below = from_lane_below(g);
    const bool head = lane == 0 || g != below;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const uint32_t run = above ? uint32_t(__builtin_ctzll(above)) + 1u : 64u - lane;
    const bool adds = head && g != kFacetNone;
    if (n_groups <= kFacetBins) {  // (uniform)
        bins[threadIdx.x] = 0;
        __syncthreads();
        if (adds) atomicAdd(&bins[g], run);
        __syncthreads();
        const uint32_t n = bins[threadIdx.x];  // (a bin at or past n_groups stays zero)
        if (n) atomicAdd(&row[threadIdx.x], n);
    } else if (adds) {
        atomicAdd(&row[g], run);
    }
}

// The facet rows of a ranked call's slots: a workgroup per page, a thread per slot, as the other slot kernels. A slot is
// alive iff it is below n_slots and its candidate is not kDeadCandidate; a dead slot carries kFacetNone, and so does a
// match at or past the map's num_docs. page_query[page] + q0 is the page's query of the call, rows + that * n_groups its row.
__global__ __launch_bounds__(256) void facet_count_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, uint32_t q0,
                                                          doc_facets_view f, uint32_t* rows) {
    __shared__ uint32_t bins[kFacetBins];
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    uint32_t g = kFacetNone;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate) g = facet_group(f, d);
    }
    facet_add(g, f.n_groups, bins, rows + uint64_t(page_query[blockIdx.x] + q0) * f.n_groups);
}

// The handle's group sizes, a thread per document, 256 per workgroup: sizes[g] += the documents of group g. An entry that
// is neither below n_groups nor kFacetNone sets *invalid and counts as none (no bin and no word past the sizes is touched).
__global__ __launch_bounds__(256) void facet_group_sizes_kernel(const uint32_t* group_of, uint64_t num_docs, uint32_t n_groups, uint32_t* sizes,
                                                                uint32_t* invalid) {
    __shared__ uint32_t bins[kFacetBins];
    const uint64_t d = uint64_t(blockIdx.x) * 256u + threadIdx.x;
    uint32_t g = kFacetNone;
    if (d < num_docs) {
        g = group_of[d];
        if (g != kFacetNone && g >= n_groups) {
            *invalid = 1u;
            g = kFacetNone;
        }
    }
    facet_add(g, n_groups, bins, sizes);
}

}  // namespace dint_dev
