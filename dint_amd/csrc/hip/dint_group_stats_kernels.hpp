// Per-group value statistics of the ranked queries: per (query, group of a facets map) the count, the sum, the minimum and the
// maximum of a column's values over the query's matches: the facets x values product. A ranked
// call already holds its match set on the device — the live slots of `cand` in front of the selection — and
// group_stats_kernel reads those slots once more, gathers one word of the map and one of the column per live slot and
// scatters a record per (query, group). As in facet_add and collapse_max, what shares a destination is reduced on chip
// first: a RUN of equal groups within a wave takes its four statistics in registers and only its last lane issues atomics,
// and with at most kFacetBins groups the page's records meet in LDS, so a page costs at most one set of global atomics per
// group present. Everything is an integer sum, minimum or maximum: the result does not depend on the order anything arrives in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_collapse_kernels.hpp"
#include "dint_value_stats_kernels.hpp"

namespace dint_dev {

// x through one DPP control, for both widths a run is scanned in (disabled lanes and rows, and sources outside the row: 0)
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t run_dpp_move(uint32_t x) {
    return __builtin_amdgcn_update_dpp(0u, x, kCtrl, kRowMask, 0xf, false);
}
template <int kCtrl, int kRowMask>
__device__ __forceinline__ unsigned long long run_dpp_move(unsigned long long x) {
    return dpp_move64<kCtrl, kRowMask>(x);
}

// run_inclusive_max's scan for any associative op: op over the lanes [first, lane] of the wave, first <= lane the first lane
// of this lane's run. EVERY lane of the wave calls it. A step joins [.., lane - s] to [lane - s + 1, lane] only if lane - s is
// in the lane's row and run, and the two cross-row moves join whole rows below: no lane enters twice, so op may be a sum.
template <typename T, typename Op>
__device__ __forceinline__ T run_inclusive_scan(T x, uint32_t lane, uint32_t first, Op op) {
    const uint32_t in_row = lane & 15u;
    T y;
    y = run_dpp_move<0x111, 0xf>(x);  // row_shr:1
    if (in_row >= 1u && lane - 1u >= first) x = op(x, y);
    y = run_dpp_move<0x112, 0xf>(x);  // row_shr:2
    if (in_row >= 2u && lane - 2u >= first) x = op(x, y);
    y = run_dpp_move<0x114, 0xf>(x);  // row_shr:4
    if (in_row >= 4u && lane - 4u >= first) x = op(x, y);
    y = run_dpp_move<0x118, 0xf>(x);  // row_shr:8
    if (in_row >= 8u && lane - 8u >= first) x = op(x, y);
    // x: op over [max(first, the row's first lane), lane]
    y = run_dpp_move<0x142, 0xa>(x);  // row_bcast:15 into rows 1 and 3
    if ((lane & 16u) && first < (lane & ~15u)) x = op(x, y);
    y = run_dpp_move<0x143, 0xc>(x);  // row_bcast:31 into rows 2 and 3
    if (lane >= 32u && first < 32u) x = op(x, y);
    return x;
}

// rec += (n, sum), rec->min = min(rec->min, mn), rec->max = max(rec->max, mx): four atomics that return nothing, so the wave
// does not wait for them. (Guarding the minimum and the maximum by a load of the record — issue the atomic only where it would
// change something — was measured and is slower: the load waits behind the atomics on its line)
__device__ __forceinline__ void group_stats_merge(value_stats_rec* rec, unsigned long long n, unsigned long long sum, uint32_t mn, uint32_t mx) {
    atomicAdd(&rec->n, n);
    atomicAdd(&rec->sum, sum);
    atomicMin(&rec->min, mn);
    atomicMax(&rec->max, mx);
}

// The group records of a ranked call's slots: a workgroup per page, a thread per slot, as the other slot kernels. A slot is
// alive iff it is below n_slots and its candidate is not kDeadCandidate; it CONTRIBUTES iff it is alive, its docID is below
// the map's num_docs and in a group there, and below the column's num_docs (the bounds first: no word past the map or the
// column is read). A lane that does not contribute — a dead slot, a match in no group, a match past the column — carries
// kFacetNone and the identities (0, 0, 0xFFFFFFFF, 0), and BREAKS runs: a grouped but unvalued document in the middle of a
// run of its group must not lend its zero to the minimum. EVERY thread reaches every barrier, every DPP move and the ballot.
// page_query[page] + q0 is the page's query of the call, recs + that * n_groups its row (the empty record where nothing has
// arrived).
//  - runs: the heads as facet_add finds them (from_lane_below and a ballot; lane 0 is always a head); a lane's run begins at
//    the highest head at or below it and ends where the next head begins or the wave ends. The run's last lane holds the
//    run's length, its 64-bit sum, its maximum and — as the maximum of the complements — its minimum, and only it issues
//    atomics.
//  - n_groups <= kFacetBins (uniform): the run ends add to the workgroup's LDS records (a 32-bit add, a 64-bit add, a min
//    and a max), and then thread t takes record t to the row iff its n is not zero (a bin at or past n_groups stays empty):
//    at most one set of global atomics per group present in the page.
//  - more groups: the run ends issue the four atomics on the row itself.
__global__ __launch_bounds__(256) void group_stats_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, uint32_t q0,
                                                          doc_facets_view f, doc_values_view values, value_stats_rec* recs) {
    __shared__ unsigned long long s_sum[kFacetBins];
    __shared__ uint32_t s_n[kFacetBins], s_min[kFacetBins], s_max[kFacetBins];
    const bool in_lds = f.n_groups <= kFacetBins;  // (uniform)
    if (in_lds) {
        s_n[threadIdx.x] = 0u;
        s_sum[threadIdx.x] = 0ull;
        s_min[threadIdx.x] = 0xFFFFFFFFu;
        s_max[threadIdx.x] = 0u;
    }
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    uint32_t g = kFacetNone, v = 0;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate && d < values.num_docs) {
            g = facet_group(f, d);
            if (g != kFacetNone) v = values.values[d];
        }
    }
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t below = from_lane_below(g);
    const bool head = lane == 0 || g != below;  // (a kFacetNone lane differs from every group: it ends the run below it)
    const unsigned long long heads = __ballot(head);                                         // (bit 0 is always set)
    const uint32_t first = 63u - uint32_t(__builtin_clzll(heads & (~0ull >> (63u - lane))));  // the highest head at or below
    const bool last = lane == kWave - 1 || ((heads >> (lane + 1u)) & 1ull);
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    const uint32_t r_max = run_inclusive_scan(v, lane, first, mx);
    const uint32_t r_min = ~run_inclusive_scan(g == kFacetNone ? 0u : ~v, lane, first, mx);
    const unsigned long long r_sum =
        run_inclusive_scan(static_cast<unsigned long long>(v), lane, first, [](unsigned long long a, unsigned long long b) { return a + b; });
    const uint32_t r_n = lane - first + 1u;
    const bool adds = last && g != kFacetNone;
    value_stats_rec* const row = recs + uint64_t(page_query[blockIdx.x] + q0) * f.n_groups;
    if (in_lds) {
        __syncthreads();  // the LDS records are empty
        if (adds) {
            atomicAdd(&s_n[g], r_n);
            atomicAdd(&s_sum[g], r_sum);
            atomicMin(&s_min[g], r_min);
            atomicMax(&s_max[g], r_max);
        }
        __syncthreads();
        const uint32_t n = s_n[threadIdx.x];
        if (n) group_stats_merge(row + threadIdx.x, n, s_sum[threadIdx.x], s_min[threadIdx.x], s_max[threadIdx.x]);
    } else if (adds) {
        group_stats_merge(row + g, r_n, r_sum, r_min, r_max);
    }
}

}  // namespace dint_dev
