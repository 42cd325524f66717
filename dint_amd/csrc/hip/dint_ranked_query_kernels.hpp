// Ranked conjunctive queries (ranked_and_query, reference include/ds2i/queries.hpp:309-385): BM25 scores of the AND
// path's matches and a per-query top-k.
//
// The scores are added term by term, in the order the AND path already visits the terms (rarest list first): after the
// rounds, and_freq_search_kernel claims the block each match falls into and ranked_gather_kernel reads the freq at the
// match's position and adds q_weight * doc_term_weight(freq, norm_len[docid]) to the match's slot. The selection then
// orders u64 keys (float bits of the score << 32 | ~docid): every score is > 0, so the keys order by score, equal scores
// by ascending docID, and a dead slot (key 0) is below every match. A query's slots are cut into runs of R keys (R a
// power of two, >= 256 and >= k); every run is sorted in LDS (topk_sort_runs_kernel), then passes of pairwise bitonic
// merges (topk_merge_kernel) keep the best R of two runs until a query has one run left. Every launch serves every query
// of the call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_query_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kRankedMaxK = DINT_RANKED_MAX_K;
constexpr float kBm25B = 0.5f;   // bm25::b  (bm25.hpp)
constexpr float kBm25K1 = 1.2f;  // bm25::k1

// BM25 as every scoring kernel computes it: q_weight * doc_term_weight(f, norm_len), doc_term_weight = f / (f + kd),
// kd = k1 * ((1 - b) + b * norm_len), added term by term from 0.0f — in binary32, in the reference's order and
// UNCONTRACTED (no fma): ranked OR, pruned ranked OR and the scores of given documents agree bit for bit because they
// all add bm25_addend's value in the same order. The pragma is lexical, so each helper carries its own.
__device__ __forceinline__ float bm25_kd(float norm_len) {
#pragma clang fp contract(off)
    return kBm25K1 * ((1.0f - kBm25B) + kBm25B * norm_len);
}
__device__ __forceinline__ float bm25_doc_term_weight(float f, float kd) {  // (what the wand data's maxima are taken over)
#pragma clang fp contract(off)
    return f / (f + kd);
}
__device__ __forceinline__ float bm25_addend(float weight, float f, float kd) {
#pragma clang fp contract(off)
    const float w = bm25_doc_term_weight(f, kd);
    return weight * w;
}
__device__ __forceinline__ float bm25_add(float sc, float weight, float f, float kd) {
#pragma clang fp contract(off)
    return sc + bm25_addend(weight, f, kd);
}

// and_query<true>'s gather with a score instead of a freq sum: every live candidate of a query that has this term finds its
// docID in its block's decoded page and adds its term's addend to its slot's score (bm25_add). term_blocks null: the rarest
// term (every live candidate is a match of its own page), where norm_len[docid] is read, once per candidate, into kden.
__global__ void ranked_gather_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, const uint32_t* term_blocks,
                                     const dint_block_ref* blocks, const uint32_t* target, const uint32_t* rank, const uint32_t* probe,
                                     const uint32_t* fprobe, const float* q_weight, const float* norm_lens, float* kden, float* score) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t c = cand[i];
    if (c == kDeadCandidate) return;
    const uint32_t q = page_query[i / kPageSlots];
    if (term_blocks && term_blocks[q] == 0) return;  // the query has no such term
    const uint32_t gb = target[i];
    const uint32_t n = blocks[gb].n;
    const uint64_t page = uint64_t(rank[gb]) * kPageSlots;
    const uint32_t pos = find_in_page(probe + page, n, c);
    if (pos == kAbsent) return;
    float kd;
    if (!term_blocks) {
        kd = bm25_kd(norm_lens[c]);
        kden[i] = kd;
    } else {
        kd = kden[i];
    }
    score[i] = bm25_add(score[i], q_weight[q], float(fprobe[page + pos]), kd);
}

// One task of the selection: query q, run a (and for a merge, run b: its best R keys are merged into run a).
struct topk_task {
    uint32_t q, a, b;
};

// (every thread of the workgroup) sorts s[0 .. n) descending, n a power of two
__device__ __forceinline__ void bitonic_sort_desc(unsigned long long* s, uint32_t n) {
    for (uint32_t size = 2; size <= n; size <<= 1)
        for (uint32_t stride = size >> 1; stride != 0; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < n / 2; t += blockDim.x) {
                const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long x = s[i], y = s[j];
                if (((i & size) == 0) == (x < y)) {  // (descending runs where i & size is clear, ascending where set)
                    s[i] = y;
                    s[j] = x;
                }
            }
            __syncthreads();
        }
}

// Stage 1: the keys of run a of query q — slots [a * R, (a + 1) * R) of the query's candidate pages, the slots past its
// last page dead — sorted descending into keys[key_base[q] + a * R ..).
__global__ void topk_sort_runs_kernel(const topk_task* tasks, const uint32_t* q_page_first, const uint32_t* q_pages,
                                      const unsigned long long* key_base, const uint32_t* cand, const float* score, uint32_t R,
                                      unsigned long long* keys) {
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
            if (c != kDeadCandidate)
                key = (static_cast<unsigned long long>(__float_as_uint(score[slot0 + e])) << 32) | (0xFFFFFFFFu - c);
        }
        s_keys[e] = key;
        any |= key != 0;
    }
    if (!__syncthreads_or(any)) {  // (no match in the run: most runs of a query with few matches)
        for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) out[e] = 0;
        return;
    }
    bitonic_sort_desc(s_keys, R);
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) out[e] = s_keys[e];
}

// A merge pass: runs a and b of query q, both sorted descending -> the best R keys of the two, sorted, in run a. Run b
// reversed behind run a is a bitonic sequence: one half-cleaner step leaves the best R in the first half (bitonic itself),
// a bitonic merge of that half sorts it.
__global__ void topk_merge_kernel(const topk_task* tasks, const unsigned long long* key_base, uint32_t R, unsigned long long* keys) {
    extern __shared__ unsigned long long s_keys[];
    const topk_task tk = tasks[blockIdx.x];
    unsigned long long* const ra = keys + key_base[tk.q] + uint64_t(tk.a) * R;
    const unsigned long long* const rb = keys + key_base[tk.q] + uint64_t(tk.b) * R;
    if (rb[0] == 0) return;  // (run b holds no match: run a is already the best of the two)
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) {
        const unsigned long long x = ra[e], y = rb[R - 1 - e];
        s_keys[e] = x > y ? x : y;
    }
    __syncthreads();
    for (uint32_t stride = R >> 1; stride != 0; stride >>= 1) {
        for (uint32_t t = threadIdx.x; t < R / 2; t += blockDim.x) {
            const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
            const unsigned long long x = s_keys[i], y = s_keys[j];
            if (x < y) {
                s_keys[i] = y;
                s_keys[j] = x;
            }
        }
        __syncthreads();
    }
    for (uint32_t e = threadIdx.x; e < R; e += blockDim.x) ra[e] = s_keys[e];
}

// out[q * k + i] = the i-th best key of query q (run 0), 0 where the query has no run
__global__ void topk_out_kernel(const unsigned long long* key_base, const uint32_t* q_pages, const unsigned long long* keys,
                                uint32_t n_queries, uint32_t k, unsigned long long* out) {
    const uint64_t x = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (x >= uint64_t(n_queries) * k) return;
    const uint32_t q = uint32_t(x / k), i = uint32_t(x % k);
    out[x] = q_pages[q] ? keys[key_base[q] + i] : 0ull;
}

}  // namespace dint_dev
