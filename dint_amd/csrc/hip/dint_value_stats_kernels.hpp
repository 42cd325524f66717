// Value statistics and range histograms of the ranked queries: per query the count, the sum, the minimum and the maximum of a
// column's values over its matches, and how many of them fall between the caller's bucket boundaries.
// A ranked call already holds its match set on the device — the live slots of `cand` in front of the selection — and
// value_stats_kernel reads those slots once more, gathers one word of the column per live slot and reduces on chip: a page
// belongs to ONE query, so the workgroup's 256 slots meet in one LDS histogram of all n_edges + 1 <= 1024 buckets and in one
// wave reduction per statistic, and a page costs at most one global add per bucket present and four atomics on its query's
// record. Everything is an integer: the result does not depend on the order the pages arrive in.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_doc_values_kernels.hpp"
#include "dint_facet_kernels.hpp"
#include "dint_wand_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kValueStatsMaxEdges = 1023;                   // DINT_VALUE_STATS_MAX_EDGES
constexpr uint32_t kValueStatsBins = kValueStatsMaxEdges + 1;    // the buckets of the largest edge set: all of them in LDS
constexpr uint32_t kValueStatsNoBucket = 0xFFFFFFFFu;            // a lane with nothing to count (no bucket is that large)

// dint_value_stats as the kernels add to it: n and sum by 64-bit adds, min and max by 32-bit atomics. The empty record is
// {0, 0, 0xFFFFFFFF, 0}: the identity of all four.
struct value_stats_rec {
    unsigned long long n, sum;
    uint32_t min, max;
};
static_assert(sizeof(value_stats_rec) == 24, "dint_value_stats is 24 bytes");

// bucket(v) = the number of edges e with e <= v, the edges strictly ascending in LDS. Branch-free, and every lane takes the
// same steps: `top` is the largest power of two <= n_edges (0: no edge, no step), uniform, and the position grows bit by
// bit — it ends at the largest p <= n_edges with edges[p - 1] <= v, since the bits below top sum to top - 1 >= n_edges - top.
// A step whose probe would lie past the edges reads edges[0] instead and moves nothing: no word past n_edges is read.
__device__ __forceinline__ uint32_t value_bucket(const uint32_t* s_edges, uint32_t n_edges, uint32_t top, uint32_t v) {
    uint32_t pos = 0;
    for (uint32_t step = top; step != 0; step >>= 1) {
        const uint32_t at = pos + step - 1u;
        const bool inside = at < n_edges;
        const uint32_t e = s_edges[inside ? at : 0u];
        pos += inside && e <= v ? step : 0u;
    }
    return pos;
}

// the sum of x over the wave, in every lane: the halves summed apart (64 lanes * 0xFFFF fits a word with room to spare)
__device__ __forceinline__ unsigned long long wave_sum64(uint32_t x) {
    const uint32_t lo = readlane(wave_inclusive_sum(x & 0xFFFFu), kWave - 1);
    const uint32_t hi = readlane(wave_inclusive_sum(x >> 16), kWave - 1);
    return (static_cast<unsigned long long>(hi) << 16) + lo;
}
// the smallest of x over the wave, in every lane
__device__ __forceinline__ uint32_t wave_min(uint32_t x) { return ~wave_max(~x); }

// The statistics and the bucket row of a ranked call's slots: a workgroup per page, a thread per slot, as the other slot
// kernels. A slot is alive iff it is below n_slots and its candidate is not kDeadCandidate; a live slot has a value iff its
// docID is below the column's num_docs (the bound first: no word past the column is read). A slot without a value carries
// the identities — bucket kValueStatsNoBucket, n 0, sum 0, min 0xFFFFFFFF, max 0 — and EVERY thread reaches every barrier,
// every DPP move and every step of the search. page_query[page] + q0 is the page's query of the call, stats + that its
// record and rows + that * (n_edges + 1) its row. edges: n_edges words on the device, strictly ascending (the host has
// checked them); n_edges == 0: no histogram, edges and rows are not touched.
//  - edges and bins: loaded / zeroed by a strided loop of the 256 threads, one barrier for both.
//  - runs, as facet_add has them: a lane is the head of a run iff it is lane 0 or its bucket differs from the lane below's;
//    the ballot of the heads gives a head its run's length; only the heads add to the LDS bins, and they add the length.
//    docIDs ascend within a page and date-like columns ascend with them: long runs. Then bin b goes to rows[b] if it is
//    not zero, again by a strided loop: at most one global add per bucket present in the page, whatever n_edges is.
//  - statistics: per wave a ballot's popcount, a DPP maximum, a minimum as the complement's maximum and the sum by halves;
//    lane 0 of every wave leaves its four in LDS, and thread 0 combines the four waves and issues one atomicMin, one
//    atomicMax and two 64-bit atomicAdd on the query's record — none if the page has no valued match.
__global__ __launch_bounds__(256) void value_stats_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, uint32_t q0,
                                                          doc_values_view values, const uint32_t* edges, uint32_t n_edges,
                                                          value_stats_rec* stats, uint32_t* rows) {
    __shared__ uint32_t s_edges[kValueStatsBins];
    __shared__ uint32_t s_bins[kValueStatsBins];
    __shared__ unsigned long long s_sum[kPageSlots / kWave];
    __shared__ uint32_t s_n[kPageSlots / kWave], s_min[kPageSlots / kWave], s_max[kPageSlots / kWave];
    const uint32_t q = page_query[blockIdx.x] + q0;
    const uint32_t n_bins = n_edges + 1u;  // (uniform; n_edges <= kValueStatsMaxEdges)
    if (n_edges != 0) {
        for (uint32_t e = threadIdx.x; e < n_edges; e += kPageSlots) s_edges[e] = edges[e];
        for (uint32_t b = threadIdx.x; b < n_bins; b += kPageSlots) s_bins[b] = 0;
    }
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    bool valued = false;
    uint32_t v = 0;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate && d < values.num_docs) {
            valued = true;
            v = values.values[d];
        }
    }
    const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    // the statistics of the wave (a lane without a value: the identities)
    const unsigned long long have = __ballot(valued);
    const uint32_t w_max = wave_max(v);
    const uint32_t w_min = wave_min(valued ? v : 0xFFFFFFFFu);
    const unsigned long long w_sum = wave_sum64(v);
    if (lane == 0) {
        s_n[wave] = uint32_t(__popcll(have));
        s_min[wave] = w_min;
        s_max[wave] = w_max;
        s_sum[wave] = w_sum;
    }
    __syncthreads();  // the edges, the zeroed bins and the waves' statistics are in LDS
    if (n_edges != 0) {  // (uniform)
        uint32_t top = 1;
        while (top * 2u <= n_edges) top *= 2u;
        const uint32_t found = value_bucket(s_edges, n_edges, top, v);
        const uint32_t b = valued ? found : kValueStatsNoBucket;
        const uint32_t below = from_lane_below(b);
        const bool head = lane == 0 || b != below;
        const unsigned long long heads = __ballot(head);
        const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1u);
        const uint32_t run = above ? uint32_t(__builtin_ctzll(above)) + 1u : kWave - lane;
        if (head && b != kValueStatsNoBucket) atomicAdd(&s_bins[b], run);
        __syncthreads();
        uint32_t* const row = rows + uint64_t(q) * n_bins;
        for (uint32_t t = threadIdx.x; t < n_bins; t += kPageSlots) {
            const uint32_t n = s_bins[t];
            if (n) atomicAdd(&row[t], n);
        }
    }
    if (threadIdx.x != 0) return;
    uint32_t n = s_n[0], mn = s_min[0], mx = s_max[0];
    unsigned long long sum = s_sum[0];
    for (uint32_t w = 1; w != kPageSlots / kWave; ++w) {
        n += s_n[w];
        mn = s_min[w] < mn ? s_min[w] : mn;
        mx = s_max[w] > mx ? s_max[w] : mx;
        sum += s_sum[w];
    }
    if (n == 0) return;  // (no valued match in the page: the record is not touched)
    value_stats_rec* const rec = stats + q;
    atomicAdd(&rec->n, static_cast<unsigned long long>(n));
    atomicAdd(&rec->sum, sum);
    atomicMin(&rec->min, mn);
    atomicMax(&rec->max, mx);
}

// Behind the selection, a thread per (query of the pass, i): keys[q * k + i] is the query's i-th best key (0 past its count),
// its low word the inverted docID. hit_values[(q0 + q) * k + i] <- the hit's value; 0 past the count and for a hit at or
// past the column (the bound first, as above).
__global__ void hit_values_kernel(const unsigned long long* keys, uint32_t n_queries, uint32_t k, uint32_t q0, doc_values_view values,
                                  uint32_t* hit_values) {
    const uint64_t x = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= uint64_t(n_queries) * k) return;
    const unsigned long long key = keys[x];
    uint32_t v = 0;
    if (key) {
        const uint32_t d = 0xFFFFFFFFu - uint32_t(key);
        if (d < values.num_docs) v = values.values[d];
    }
    hit_values[uint64_t(q0) * k + x] = v;
}

}  // namespace dint_dev
