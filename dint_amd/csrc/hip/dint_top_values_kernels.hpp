// The top values and the distinct count of a column over the matches of the ranked queries: per
// query the number of different values among its valued matches and the n_top values that occur most, with their counts. The
// key space is not known in advance — a column is an arbitrary u32 per document — so the matches are aggregated in an
// open-addressing hash table per query: 64-bit words `value << 32 | count`, 0 an empty word (a present value has count >= 1,
// so value 0 is representable), linear probing. A query of P pages owns 2 * P * 256 words: distinct <= valued matches <=
// slots, so the load never exceeds 1/2. top_values_count_kernel fills the tables, a page at a time through a page-local LDS
// table; top_values_sort_runs_kernel turns runs of table words into sorted keys `count << 32 | ~value`, which the ranked
// selection's merge and output kernels (dint_ranked_query_kernels.hpp) order as they order any keys. Every quantity is an
// integer count: the result is exact, does not depend on the order the pages arrive in and equals a sort-and-count's.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_doc_values_kernels.hpp"
#include "dint_facet_kernels.hpp"
#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kTopValuesMax = DINT_TOP_VALUES_MAX;
constexpr uint32_t kTopValuesPageWords = 2 * kPageSlots;  // a page's LDS table, and a page's share of its query's table

// murmur3's finaliser: every input bit reaches every output bit
__device__ __forceinline__ uint32_t top_values_mix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

// n more of value v into the table of `cap` words: from the value's start slot — its mix scaled to the capacity by
// multiply-high — linearly, wrapping at the capacity. Each probe is ONE compare-and-swap against the empty word, and the lane
// acts only on what the atomic returned (a plain load of a word another XCD has just written may be stale): 0 — the value is
// inserted; the same value — a 64-bit add of n (a query has < 2^32 matches: nothing carries into the value); another value —
// the next slot. No lane waits for another. The loop ends after `cap` probes: at a load of at most 1/2 that never happens,
// and a lane that gets there sets *overflow, which the host turns into an error. -> true iff the value was inserted.
__device__ __forceinline__ bool top_values_add(unsigned long long* table, uint32_t cap, uint32_t v, uint32_t n, uint32_t* overflow) {
    const unsigned long long word = (static_cast<unsigned long long>(v) << 32) | n;
    uint32_t at = __umulhi(top_values_mix(v), cap);
    for (uint32_t probe = 0; probe != cap; ++probe) {
        const unsigned long long old = atomicCAS(&table[at], 0ull, word);
        if (old == 0ull) return true;
        if (uint32_t(old >> 32) == v) {
            atomicAdd(&table[at], static_cast<unsigned long long>(n));
            return false;
        }
        at = at + 1u == cap ? 0u : at + 1u;
    }
    atomicOr(overflow, 1u);
    return false;
}

// The count over a ranked call's slots: a workgroup per page, a thread per slot, as the other slot kernels. A slot is alive
// iff it is below n_slots and its candidate is not kDeadCandidate; a live slot has a value iff its docID is below the
// column's num_docs (the bound first: no word past the column is read). page_query[page] = p is the page's query of the pass
// and p + q0 its query of the call: its table is the q_pages[p] * 512 words of `table` from word q_page_first[p] * 512 on
// (zero when the kernel begins), its counters are n[p + q0] and distinct[p + q0].
//  - runs of equal values within a wave merge first, as percentile_count merges digits: a lane is a head iff it is lane 0 or
//    its (valued, value) differs from the lane below's, and the ballot of the heads gives a head its run's length;
//  - the valued heads add their run to the page's LDS table (512 words for at most 256 values);
//  - behind the barrier thread t takes the LDS words t and t + 256 to the query's table: a page sends each of its distinct
//    values to memory once.
// The valued lanes and the inserts are counted per wave from a ballot, one add each. EVERY thread reaches every barrier,
// every ballot and every cross-lane move; a lane without a value adds nowhere.
__global__ __launch_bounds__(256) void top_values_count_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, uint32_t q0,
                                                               doc_values_view values, const uint32_t* q_page_first, const uint32_t* q_pages,
                                                               unsigned long long* table, uint32_t* n, uint32_t* distinct,
                                                               uint32_t* overflow) {
    __shared__ unsigned long long s_table[kTopValuesPageWords];
    for (uint32_t b = threadIdx.x; b < kTopValuesPageWords; b += kPageSlots) s_table[b] = 0ull;
    const uint32_t p = page_query[blockIdx.x];
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    uint32_t valued = 0, v = 0;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate && d < values.num_docs) {
            valued = 1;
            v = values.values[d];
        }
    }
    __syncthreads();  // the empty table is in LDS
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint32_t v_below = from_lane_below(v), valued_below = from_lane_below(valued);
    const bool head = lane == 0 || v != v_below || valued != valued_below;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1u);
    const uint32_t run = above ? uint32_t(__builtin_ctzll(above)) + 1u : kWave - lane;
    const unsigned long long with_value = __ballot(valued != 0);
    if (lane == 0 && with_value) atomicAdd(&n[p + q0], uint32_t(__builtin_popcountll(with_value)));
    if (head && valued) (void)top_values_add(s_table, kTopValuesPageWords, v, run, overflow);
    __syncthreads();
    unsigned long long* const q_table = table + uint64_t(q_page_first[p]) * kTopValuesPageWords;
    const uint32_t cap = q_pages[p] * kTopValuesPageWords;  // (the host refuses a query whose capacity does not fit a word)
    for (uint32_t b = threadIdx.x; b < kTopValuesPageWords; b += kPageSlots) {  // (two turns, uniform)
        const unsigned long long w = s_table[b];
        bool inserted = false;
        if (w) inserted = top_values_add(q_table, cap, uint32_t(w >> 32), uint32_t(w), overflow);
        const unsigned long long fresh = __ballot(inserted);
        if (lane == 0 && fresh) atomicAdd(&distinct[p + q0], uint32_t(__builtin_popcountll(fresh)));
    }
}

// Stage 1 of the selection over the tables, beside topk_sort_runs_kernel: the keys of run a of query q — the words
// [a * R, (a + 1) * R) of the query's table, the words past its capacity empty — sorted descending into
// keys[key_base[q] + a * R ..). A word's key is count << 32 | (0xFFFFFFFF - value), an empty word's 0: the keys order by
// count descending, equal counts by value ascending, keys of distinct values are distinct, and an empty word is below
// every value (a count is >= 1).
__global__ void top_values_sort_runs_kernel(const topk_task* tasks, const uint32_t* q_page_first, const uint32_t* q_pages,
                                            const unsigned long long* key_base, const unsigned long long* table, uint32_t R,
                                            unsigned long long* keys) {
    extern __shared__ unsigned long long s_keys[];
    const topk_task tk = tasks[blockIdx.x];
    const uint64_t cap = uint64_t(q_pages[tk.q]) * kTopValuesPageWords;
    const uint64_t word0 = uint64_t(q_page_first[tk.q]) * kTopValuesPageWords + uint64_t(tk.a) * R;
    unsigned long long* const out = keys + key_base[tk.q] + uint64_t(tk.a) * R;
    int any = 0;
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) {
        unsigned long long key = 0;
        if (uint64_t(tk.a) * R + e < cap) {
            const unsigned long long w = table[word0 + e];
            if (w) key = (w << 32) | (0xFFFFFFFFu - uint32_t(w >> 32));
        }
        s_keys[e] = key;
        any |= key != 0;
    }
    if (!__syncthreads_or(any)) {  // (no value in the run: half the runs at the least)
        for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) out[e] = 0;
        return;
    }
    bitonic_sort_desc(s_keys, R);
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) out[e] = s_keys[e];
}

}  // namespace dint_dev
