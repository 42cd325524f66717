// Collapsed ranked queries: of every document group a query matches, only its best document reaches the selection
// (DESIGN.md 4d-collapse). A ranked call holds its match set on the device — the live slots of `cand` with their scores in
// front of ranked_topk — and a document's key is the one the selection sorts by (score bits, then the inverted docID).
// collapse_best_kernel takes the maximum key per (query, group) into a table, collapse_keep_kernel kills every grouped slot
// whose key is not its group's maximum, and behind the selection collapse_hits_kernel names the group of every hit and the
// matches that group holds (the facet rows' entry). A 64-bit maximum is order-independent: the answer is exact and the same
// from run to run.
// The table is again a scatter onto few addresses, so what shares a destination is reduced on chip first, as facet_add
// does: a run of equal groups within a wave takes a segmented maximum in registers and only its last lane issues an atomic,
// and with at most kFacetBins groups the page's maxima meet in LDS, so a page costs at most one global atomic per group
// present.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_facet_kernels.hpp"

namespace dint_dev {

// the selection's key of a live slot (topk_sort_runs_kernel builds the same): never 0, the docID is below 0xFFFFFFFF
__device__ __forceinline__ unsigned long long collapse_key(float score, uint32_t d) {
    return (static_cast<unsigned long long>(__float_as_uint(score)) << 32) | (0xFFFFFFFFu - d);
}

// a 64-bit value through one DPP control, half by half (disabled lanes and rows, and sources outside the row: 0)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned long long dpp_move64(unsigned long long x) {
    const uint32_t lo = __builtin_amdgcn_update_dpp(0u, uint32_t(x), kCtrl, kRowMask, 0xf, false);
    const uint32_t hi = __builtin_amdgcn_update_dpp(0u, uint32_t(x >> 32), kCtrl, kRowMask, 0xf, false);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// The inclusive maximum of x over the lanes [first, lane] of the wave, first <= lane the first lane of this lane's run
// (runs are consecutive lanes, so every lane of [first, lane] has the same first). EVERY lane of the wave calls it. Four
// log-steps inside a row of 16 (row_shr: a lane takes the value s lanes below if that lane is in its row and in its run),
// then the two cross-row moves of a wave scan: row_bcast:15 hands lane 15 / 47 to the row above for the runs that began
// below that row, row_bcast:31 hands lane 31 to the upper half for the runs that began in the lower one.
__device__ __forceinline__ unsigned long long run_inclusive_max(unsigned long long x, uint32_t lane, uint32_t first) {
    auto mx = [](unsigned long long a, unsigned long long b) { return a > b ? a : b; };
    const uint32_t in_row = lane & 15u;
    unsigned long long y;
    y = dpp_move64<0x111, 0xf>(x);  // row_shr:1
    if (in_row >= 1u && lane - 1u >= first) x = mx(x, y);
    y = dpp_move64<0x112, 0xf>(x);  // row_shr:2
    if (in_row >= 2u && lane - 2u >= first) x = mx(x, y);
    y = dpp_move64<0x114, 0xf>(x);  // row_shr:4
    if (in_row >= 4u && lane - 4u >= first) x = mx(x, y);
    y = dpp_move64<0x118, 0xf>(x);  // row_shr:8
    if (in_row >= 8u && lane - 8u >= first) x = mx(x, y);
    // x: the maximum over [max(first, the row's first lane), lane]
    y = dpp_move64<0x142, 0xa>(x);  // row_bcast:15 into rows 1 and 3
    if ((lane & 16u) && first < (lane & ~15u)) x = mx(x, y);
    y = dpp_move64<0x143, 0xc>(x);  // row_bcast:31 into rows 2 and 3
    if (lane >= 32u && first < 32u) x = mx(x, y);
    return x;
}

// best_row[g] = max(best_row[g], key) over the threads of the workgroup whose group is g, for every g != kFacetNone. EVERY
// thread of a 256-thread workgroup calls it (the DPP moves read every lane, and the LDS form has barriers); a thread with
// nothing to offer carries kFacetNone. g < n_groups or g == kFacetNone; key != 0 where g is a group. bins: kFacetBins
// 64-bit words of LDS.
//  - runs: the heads as facet_add finds them (from_lane_below and a ballot); a lane's run begins at the highest head at
//    or below it and ends where the next head begins or the wave ends. The run's last lane holds the run's maximum after
//    run_inclusive_max, and only it issues an atomic. kFacetNone breaks runs and adds nothing.
//  - n_groups <= kFacetBins: the run ends take the maximum into the workgroup's LDS table, and then thread t takes bin t
//    into best_row[t] if it is not zero: at most one global atomic per group present in the workgroup.
//  - more groups: the run ends take the maximum into the row itself.
__device__ __forceinline__ void collapse_max(uint32_t g, unsigned long long key, uint32_t n_groups, unsigned long long* bins,
                                             unsigned long long* best_row) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t below = from_lane_below(g);
    const bool head = lane == 0 || g != below;
    const unsigned long long heads = __ballot(head);                                         // (bit 0 is always set)
    const uint32_t first = 63u - uint32_t(__builtin_clzll(heads & (~0ull >> (63u - lane))));  // the highest head at or below
    const bool last = lane == 63u || ((heads >> (lane + 1u)) & 1ull);
    const unsigned long long m = run_inclusive_max(key, lane, first);
    const bool offers = last && g != kFacetNone;
    if (n_groups <= kFacetBins) {  // (uniform)
        bins[threadIdx.x] = 0ull;
        __syncthreads();
        if (offers) atomicMax(&bins[g], m);
        __syncthreads();
        const unsigned long long b = bins[threadIdx.x];  // (a bin at or past n_groups stays zero)
        if (b) atomicMax(&best_row[threadIdx.x], b);
    } else if (offers) {
        atomicMax(&best_row[g], m);
    }
}

// The best key of every (query, group) of a ranked call's slots: a workgroup per page, a thread per slot, as the other slot
// kernels. A dead slot and a match in no group (kFacetNone in the map, or at or past its num_docs) carry kFacetNone.
// slot_group[i] <- the slot's group, so that collapse_keep_kernel does not gather the map again. page_query[page] + q0 is the
// page's query of the call, best + that * n_groups its row (zero where no key has arrived: a live key is never 0).
__global__ __launch_bounds__(256) void collapse_best_kernel(const uint32_t* cand, const float* score, uint64_t n_slots,
                                                            const uint32_t* page_query, uint32_t q0, doc_facets_view f,
                                                            unsigned long long* best, uint32_t* slot_group) {
    __shared__ unsigned long long bins[kFacetBins];
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    uint32_t g = kFacetNone;
    unsigned long long key = 0ull;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate) {
            g = facet_group(f, d);
            if (g != kFacetNone) key = collapse_key(score[i], d);
        }
        slot_group[i] = g;
    }
    collapse_max(g, key, f.n_groups, bins, best + uint64_t(page_query[blockIdx.x] + q0) * f.n_groups);
}

// A live slot in a group whose key is not the group's best dies; keys are unique within a query (docIDs are), so exactly
// one slot per matched group survives. The survivors — the ungrouped matches among them, which stand for themselves — are
// counted into collapsed[the page's query]: a ballot and one add per wave, a page belongs to one query.
__global__ __launch_bounds__(256) void collapse_keep_kernel(uint32_t* cand, const float* score, const uint32_t* slot_group, uint64_t n_slots,
                                                            const uint32_t* page_query, uint32_t q0, uint32_t n_groups,
                                                            const unsigned long long* best, unsigned long long* collapsed) {
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    const uint32_t q = page_query[blockIdx.x] + q0;
    bool kept = false;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate) {
            const uint32_t g = slot_group[i];
            kept = g == kFacetNone || collapse_key(score[i], d) == best[uint64_t(q) * n_groups + g];
            if (!kept) cand[i] = kDeadCandidate;
        }
    }
    const unsigned long long keeps = __ballot(kept);
    if ((threadIdx.x & 63u) == 0 && keeps) atomicAdd(&collapsed[q], static_cast<unsigned long long>(__popcll(keeps)));
}

// Behind the selection, a thread per (query of the pass, i): keys[q * k + i] is the query's i-th best key (0 past its kept
// documents). hit_groups / hit_group_matches at (q0 + q) * k + i <- the hit's group and the matches of the query in that
// group (the call's facet row, counted over every match before anything was killed); an ungrouped hit: kFacetNone and 1;
// past the count: kFacetNone and 0.
__global__ void collapse_hits_kernel(const unsigned long long* keys, uint32_t n_queries, uint32_t k, uint32_t q0, doc_facets_view f,
                                     const uint32_t* rows, uint32_t* hit_groups, uint32_t* hit_group_matches) {
    const uint64_t x = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= uint64_t(n_queries) * k) return;
    const uint64_t q = q0 + x / k;
    const unsigned long long key = keys[x];
    uint32_t g = kFacetNone, n = 0;
    if (key) {
        g = facet_group(f, 0xFFFFFFFFu - uint32_t(key));
        n = g == kFacetNone ? 1u : rows[q * f.n_groups + g];
    }
    hit_groups[q * k + x % k] = g;
    hit_group_matches[q * k + x % k] = n;
}

}  // namespace dint_dev
