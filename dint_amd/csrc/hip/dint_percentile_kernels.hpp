// Exact percentiles of a column's values over the matches of the ranked queries: per query and
// requested rank the value at that rank of the ascending sort of its valued matches. A ranked call already holds its match
// set on the device — the live slots of `cand` in front of the selection — and a percentile is a SELECTION over those slots,
// not a reduction: an MSB-first radix select with 8-bit digits, four rounds, each a histogram over the slots
// (percentile_hist_kernel) and a scan of the histogram that fixes the next byte of the answer (percentile_resolve_kernel).
// A round reads what the round before it wrote — the prefix and the remaining rank of every (query, percentile) — from
// device memory: nothing returns to the host between the rounds. Everything is an integer count: the result is exact, does
// not depend on the order the pages arrive in and equals a sort's, bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_doc_values_kernels.hpp"
#include "dint_facet_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kPercentilesMax = 16;    // DINT_PERCENTILES_MAX
constexpr uint32_t kPercentileBins = 256;   // one digit of the select: a counter row is 1 KiB
constexpr uint32_t kPercentileRounds = 4;   // 32-bit values, a byte a round

// The select of one (query, percentile) between the rounds: the bytes of the answer fixed so far (after round r its top
// 8 * (r + 1) bits, in the low bits of the word) and the rank that remains among the values that begin with them.
struct percentile_state {
    uint32_t prefix, rank;
};

constexpr uint32_t kPercentileNoDigit = 0xFFFFFFFFu;  // a lane with nothing to count (no digit is that large)

// One count of `key` (a digit, or kPercentileNoDigit) per lane into the 256 bins, by runs as facet_add has them: a lane is the
// head of a run iff it is lane 0 or its key differs from the lane below's, the ballot of the heads gives a head its run's
// length, and only the heads add to LDS, the length. DocIDs ascend within a page, so a column that ascends with them gives
// long runs of equal digits, and in the rounds behind the first the lanes outside a prefix are one run that adds nothing.
// EVERY lane of the wave must call it.
__device__ __forceinline__ void percentile_count(uint32_t* bins, uint32_t key, uint32_t lane) {
    const uint32_t below = from_lane_below(key);
    const bool head = lane == 0 || key != below;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == kWave - 1 ? 0ull : heads >> (lane + 1u);
    const uint32_t run = above ? uint32_t(__builtin_ctzll(above)) + 1u : kWave - lane;
    if (head && key != kPercentileNoDigit) atomicAdd(&bins[key], run);
}

// Round `round` of the select over a ranked call's slots: a workgroup per page, a thread per slot, as the other slot kernels.
// A slot is alive iff it is below n_slots and its candidate is not kDeadCandidate; a live slot has a value iff its docID is
// below the column's num_docs (the bound first: no word past the column is read). page_query[page] + q0 = q is the page's
// query of the call; its rows are rows[(q * n_p + j) * 256 ..], j < n_p, and its states state[q * n_p + j].
//  - round 0 counts the top byte of every value into ONE 256-bin LDS histogram — it does not depend on the rank, so all the
//    percentiles of a query share row j = 0;
//  - rounds 1 to 3 load the query's n_p prefixes into LDS, and for each of them (a loop that is uniform across the workgroup)
//    the lanes whose value's higher bits equal the prefix count their digit into that percentile's 256 bins: 16 KiB of LDS.
// EVERY thread reaches every barrier and every cross-lane move of percentile_count; a lane without a value counts nowhere.
// The bins go to the rows by a strided loop, at most one global add per non-zero bin. The rows are zero when the round
// begins (percentile_launch).
__global__ __launch_bounds__(256) void percentile_hist_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, uint32_t q0,
                                                              doc_values_view values, uint32_t round, uint32_t n_p,
                                                              const percentile_state* state, uint32_t* rows) {
    __shared__ uint32_t s_bins[kPercentilesMax * kPercentileBins];
    __shared__ uint32_t s_prefix[kPercentilesMax];
    const uint32_t q = page_query[blockIdx.x] + q0;
    const uint32_t n_bins = (round == 0 ? 1u : n_p) * kPercentileBins;  // (uniform; n_p <= kPercentilesMax)
    for (uint32_t b = threadIdx.x; b < n_bins; b += kPageSlots) s_bins[b] = 0;
    if (round != 0 && threadIdx.x < n_p) s_prefix[threadIdx.x] = state[uint64_t(q) * n_p + threadIdx.x].prefix;
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
    __syncthreads();  // the zeroed bins and the prefixes are in LDS
    const uint32_t shift = 24u - 8u * round;
    const uint32_t digit = (v >> shift) & 0xFFu;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    if (round == 0) {
        percentile_count(s_bins, valued ? digit : kPercentileNoDigit, lane);
    } else {
        const uint32_t high = v >> (shift + 8u);  // (round >= 1: the shift is at most 24)
        for (uint32_t j = 0; j != n_p; ++j)
            percentile_count(s_bins + j * kPercentileBins, valued && high == s_prefix[j] ? digit : kPercentileNoDigit, lane);
    }
    __syncthreads();
    uint32_t* const row = rows + uint64_t(q) * n_p * kPercentileBins;
    for (uint32_t b = threadIdx.x; b < n_bins; b += kPageSlots) {
        const uint32_t n = s_bins[b];
        if (n) atomicAdd(&row[b], n);
    }
}

// Behind a round's histogram: a wave per (query of the pass, percentile) — wave w is query q0 + w / n_p, percentile w % n_p;
// a wave past n_ids * n_p leaves whole, and there is no barrier. Lane l takes the four adjacent bins 4 l .. 4 l + 3 of the
// row (round 0: the query's shared row) and the wave sums the lanes' partial sums inclusively; the first lane whose running
// count exceeds the remaining rank holds the digit, and finds it among its four bins. That lane appends the digit to the
// prefix and takes the count below it off the rank.
//  - round 0 derives n_q as the row's total, writes value_n[q] (percentile 0's wave) and starts from the rank
//    ((n_q - 1) * per_million[j]) / 1000000 in 64 bits; the later rounds start from the state. A query has fewer than 2^32
//    matches: every counter and rank fits a word.
//  - n_q == 0: no lane exceeds the rank; the state stays {0, 0} and the answer is 0.
//  - after round 3 the prefix is the answer: out[q * n_p + j].
//  - clear (rounds 1 and 2; never round 0, whose row n_p waves read): the wave zeroes the row it alone has read, for the
//    next round's histogram.
__global__ __launch_bounds__(256) void percentile_resolve_kernel(uint32_t* rows, uint32_t q0, uint32_t n_ids, uint32_t n_p, uint32_t round,
                                                                 const uint32_t* per_million, percentile_state* state, uint32_t* value_n,
                                                                 uint32_t* out, uint32_t clear) {
    const uint32_t w = blockIdx.x * (256u / kWave) + threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    if (w >= n_ids * n_p) return;  // (uniform in the wave; n_ids * n_p <= 2^16)
    const uint32_t q = q0 + w / n_p, j = w % n_p;
    const uint64_t rec = uint64_t(q) * n_p + j;
    uint4* const row = reinterpret_cast<uint4*>(rows + (round == 0 ? uint64_t(q) * n_p : rec) * kPercentileBins);
    const uint4 c = row[lane];
    if (clear) row[lane] = uint4{0u, 0u, 0u, 0u};
    const uint32_t part = c.x + c.y + c.z + c.w;
    const uint32_t incl = wave_inclusive_sum(part);
    uint32_t prefix = 0, rank = 0;
    if (round == 0) {
        const uint32_t n_q = readlane(incl, kWave - 1);
        if (n_q) rank = uint32_t((uint64_t(n_q - 1u) * per_million[j]) / 1000000u);
        if (j == 0 && lane == 0) value_n[q] = n_q;
    } else {
        const percentile_state st = state[rec];
        prefix = st.prefix;
        rank = st.rank;
    }
    const unsigned long long past = __ballot(incl > rank);
    if (past == 0) {  // (no valued match: uniform)
        if (lane == 0 && round == kPercentileRounds - 1) out[rec] = 0;
        return;
    }
    if (lane != uint32_t(__builtin_ctzll(past))) return;
    uint32_t r = rank - (incl - part), d = 0;  // the rank among this lane's four bins: r < part
    if (r >= c.x) {
        r -= c.x, d = 1;
        if (r >= c.y) {
            r -= c.y, d = 2;
            if (r >= c.z) r -= c.z, d = 3;
        }
    }
    prefix = (prefix << 8) | (lane * 4u + d);
    state[rec] = percentile_state{prefix, r};
    if (round == kPercentileRounds - 1) out[rec] = prefix;
}

}  // namespace dint_dev
