// Document values: one u32 per document on the device (dint_doc_values_create), the ranked queries sorted by it and the
// value-range filter built from it. A sorted call holds its match set as every ranked call does — the
// live slots of `cand` with their scores in front of ranked_topk — and the selection orders opaque 64-bit keys, descending;
// only its first stage knows what a key is made of. Here the key of document d is
//     K(d) = (order == ASC ? ~v(d) : v(d)) << 32 | (0xFFFFFFFF - d),      v(d) = 0 for a d at or past the column's end,
// so the larger (ASC: the smaller) value comes first and equal values go by ascending docID in both orders. 0xFFFFFFFF is no
// docID: a live key is never 0, the key of a dead slot. Four kernels: the cut behind a cursor (value_after_kernel), stage 1 of
// the selection on K (topk_sort_runs_by_value_kernel; the merges and the output are the score selection's, unedited), the
// scores of the selected hits (sorted_hits_kernel: a key has no room for them) and the bitmap of a value interval
// (values_in_range_bits_kernel). Everything is an integer comparison: no tolerance, the same answer from run to run.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kSortAsc = 1;  // DINT_SORT_ASC (DINT_SORT_DESC: 0)

// A column as the kernels see it.
struct doc_values_view {
    const uint32_t* values;  // max(1, num_docs) words
    uint32_t num_docs;
};
// v(d). The bound first: no word past the column is read.
__device__ __forceinline__ uint32_t doc_value(const doc_values_view& v, uint32_t d) { return d < v.num_docs ? v.values[d] : 0u; }
// K(d)
__device__ __forceinline__ unsigned long long value_key(const doc_values_view& v, uint32_t order, uint32_t d) {
    const uint32_t x = doc_value(v, d);
    return (static_cast<unsigned long long>(order == kSortAsc ? ~x : x) << 32) | (0xFFFFFFFFu - d);
}

// page_after_kernel on K(d): a workgroup per page, a thread per slot. page_query[page] + q0 is the page's query of the call,
// after_key[that] its cursor's key and after_set[that] whether it has a cursor at all — every 64-bit pattern is a legitimate
// key here (~0: value 0xFFFFFFFF, document 0, descending), so none can stand for "from the start". No cursor: the workgroup
// returns — a uniform branch. Otherwise a live slot whose key is at or above the cursor's dies, and the dead are counted into
// skipped[the page's query]: a ballot and at most one add per wave, a page belongs to one query.
__global__ __launch_bounds__(256) void value_after_kernel(uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, uint32_t q0,
                                                          doc_values_view values, uint32_t order, const unsigned long long* after_key,
                                                          const uint32_t* after_set, unsigned long long* skipped) {
    const uint32_t q = page_query[blockIdx.x] + q0;
    if (after_set[q] == 0) return;  // (uniform)
    const unsigned long long after = after_key[q];
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    bool killed = false;
    if (i < n_slots) {
        const uint32_t d = cand[i];
        if (d != kDeadCandidate) {
            killed = value_key(values, order, d) >= after;
            if (killed) cand[i] = kDeadCandidate;
        }
    }
    const unsigned long long kills = __ballot(killed);
    if ((threadIdx.x & 63u) == 0 && kills) atomicAdd(&skipped[q], static_cast<unsigned long long>(__popcll(kills)));
}

// Stage 1 of the selection by value: topk_sort_runs_kernel with K(d) in place of the score key — the keys of run a of query
// q, the slots past the query's last page dead, sorted descending into keys[key_base[q] + a * R ..).
__global__ void topk_sort_runs_by_value_kernel(const topk_task* tasks, const uint32_t* q_page_first, const uint32_t* q_pages,
                                               const unsigned long long* key_base, const uint32_t* cand, doc_values_view values,
                                               uint32_t order, uint32_t R, unsigned long long* keys) {
    extern __shared__ unsigned long long s_keys[];
    const topk_task tk = tasks[blockIdx.x];
    const uint64_t n_q = uint64_t(q_pages[tk.q]) * kPageSlots;
    const uint64_t slot0 = uint64_t(q_page_first[tk.q]) * kPageSlots + uint64_t(tk.a) * R;
    unsigned long long* const out = keys + key_base[tk.q] + uint64_t(tk.a) * R;
    int any = 0;
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) {
        unsigned long long key = 0;
        if (uint64_t(tk.a) * R + e < n_q) {
            const uint32_t c = cand[slot0 + e];
            if (c != kDeadCandidate) key = value_key(values, order, c);
        }
        s_keys[e] = key;
        any |= key != 0;
    }
    if (!__syncthreads_or(any)) {  // (no match in the run)
        for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) out[e] = 0;
        return;
    }
    bitonic_sort_desc(s_keys, R);
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) out[e] = s_keys[e];
}

// The scores of the selected hits, behind the selection: a workgroup per page, a thread per slot. topk_out[ql * k ..) are the
// k keys the selection kept for the page's query ql of the pass (page_query[page]), descending, zero past the count; they are
// staged in LDS (k <= kRankedMaxK: at most 8 KiB). Every live slot rebuilds its K(d) and binary-searches the run: keys are
// unique within a query (a docID has one live slot), so a slot that finds itself at position i is hit i and stores its score
// to hit_scores[(ql + q0) * k + i]. A slot below the run's last non-zero key leaves after one compare. No atomics: every
// output word has at most one writer.
__global__ __launch_bounds__(256) void sorted_hits_kernel(const uint32_t* cand, const float* score, uint64_t n_slots,
                                                          const uint32_t* page_query, uint32_t q0, doc_values_view values, uint32_t order,
                                                          const unsigned long long* topk_out, uint32_t k, float* hit_scores) {
    __shared__ unsigned long long s_run[kRankedMaxK];
    __shared__ uint32_t s_n;
    const uint32_t ql = page_query[blockIdx.x];
    const unsigned long long* const run = topk_out + uint64_t(ql) * k;
    if (threadIdx.x == 0) s_n = 0;
    for (uint32_t e = threadIdx.x; e < k; e += blockDim.x) s_run[e] = run[e];
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < k; e += blockDim.x)
        if (s_run[e] != 0 && (e + 1 == k || s_run[e + 1] == 0)) s_n = e + 1;  // (one e: the run is descending, its zeros last)
    __syncthreads();
    const uint32_t n = s_n;
    if (n == 0) return;  // (uniform: the query has no hit)
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t d = cand[i];
    if (d == kDeadCandidate) return;
    const unsigned long long key = value_key(values, order, d);
    if (key < s_run[n - 1]) return;  // behind the page's last hit
    uint32_t lo = 0, hi = n;  // the first position whose key is <= this one
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (s_run[mid] > key)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo < n && s_run[lo] == key) hit_scores[(uint64_t(ql) + q0) * k + lo] = score[i];
}

// The bitmap of the documents d < num_docs with lo <= v(d) <= hi, straight into a filter handle's words: a thread per
// document, the wave's ballot is the word, stored by the wave's first lane. A document past num_docs votes 0, so the last
// word needs no mask. lo > hi: nobody votes.
__global__ __launch_bounds__(256) void values_in_range_bits_kernel(doc_values_view values, uint32_t lo, uint32_t hi, uint64_t n_words,
                                                                   uint64_t* bits) {
    const uint64_t d = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    bool in = false;
    if (d < values.num_docs) {
        const uint32_t x = values.values[d];
        in = lo <= x && x <= hi;
    }
    const unsigned long long word = __ballot(in);
    if ((threadIdx.x & 63u) == 0 && (d >> 6) < n_words) bits[d >> 6] = word;
}

}  // namespace dint_dev
