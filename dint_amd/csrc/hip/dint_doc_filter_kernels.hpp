// Document-filter ranked queries: the ranked OR and ranked AND calls restricted to the documents of a bitmap over the docID
// space, one per call. Two halves:
//  - the filter handle's construction (dint_doc_filter_create): a rank directory of the bitmap (exclusive prefix popcounts,
//    an entry per 64-bit word, so the set bits of ANY docID interval cost two entries and two words), from it a flag per
//    block of the index — live iff the filter holds a document of the block's [base, max] — and the exclusive prefix count
//    of the live blocks (live_before). Both prefix sums are one scan: a wave64 DPP scan (wave_inclusive_sum), the four
//    waves of a workgroup through LDS, the workgroups through a partials array that one workgroup scans and a last launch
//    adds back.
//  - the query kernels: the host plans only the live blocks (a list's pages are its live blocks, in order), so a block
//    position pos of a list whose first block is fb lies in page term_page + live_before[fb + pos] - live_before[fb];
//    what the live blocks hold outside the filter dies here before it costs anything.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_ranked_or_query_kernels.hpp"

namespace dint_dev {

constexpr uint32_t kScanThreads = 256;  // a workgroup of the scans: four waves, an element per thread

// ---- the scan ---------------------------------------------------------------------------------------------------------

// The exclusive prefix sum of one value per thread over a workgroup of kScanThreads; *total: the workgroup's sum.
// wave_totals: kScanThreads / 64 words of LDS. Every thread of the workgroup calls it (the DPP scan reads every lane), and
// may call it again at once.
__device__ __forceinline__ uint32_t workgroup_exclusive_sum(uint32_t x, uint32_t* wave_totals, uint32_t* total) {
    const uint32_t incl = wave_inclusive_sum(x);
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 63u) wave_totals[wave] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
    for (uint32_t w = 0; w != kScanThreads / 64; ++w) {
        const uint32_t t = wave_totals[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();  // (the totals are read: the next call may write them)
    *total = all;
    return before + incl - x;
}

// Workgroup level of the rank directory: out[i] <- the set bits of words [256 * blockIdx.x, i), partials[blockIdx.x] <-
// those of the workgroup's words.
__global__ __launch_bounds__(kScanThreads) void filter_word_rank_kernel(const uint64_t* bits, uint64_t n_words, uint32_t* out,
                                                                        uint32_t* partials) {
    __shared__ uint32_t wave_totals[kScanThreads / 64];
    const uint64_t i = uint64_t(blockIdx.x) * kScanThreads + threadIdx.x;
    const uint32_t x = i < n_words ? uint32_t(__popcll(bits[i])) : 0u;
    uint32_t total;
    const uint32_t before = workgroup_exclusive_sum(x, wave_totals, &total);
    if (i < n_words) out[i] = before;
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// Grid level: partials[0 .. n) <- their exclusive prefix sums, *total <- their sum. ONE workgroup walks them, 256 at a time.
__global__ __launch_bounds__(kScanThreads) void scan_partials_kernel(uint32_t* partials, uint64_t n, uint32_t* total) {
    __shared__ uint32_t wave_totals[kScanThreads / 64];
    uint32_t carry = 0;
    for (uint64_t at = 0; at < n; at += kScanThreads) {  // (uniform)
        const uint64_t i = at + threadIdx.x;
        const uint32_t x = i < n ? partials[i] : 0u;
        uint32_t sum;
        const uint32_t before = workgroup_exclusive_sum(x, wave_totals, &sum);
        if (i < n) partials[i] = carry + before;
        carry += sum;
    }
    if (threadIdx.x == 0) *total = carry;
}

// ... and the add: out[i] += what the workgroups before i's counted. (out[n] is scan_partials_kernel's total.)
__global__ __launch_bounds__(kScanThreads) void scan_add_kernel(uint32_t* out, uint64_t n, const uint32_t* partials) {
    const uint64_t i = uint64_t(blockIdx.x) * kScanThreads + threadIdx.x;
    if (i < n) out[i] += partials[blockIdx.x];
}

// The set bits below docID x (x <= num_docs): two reads whatever x. rank: the directory, an entry per word and one past the
// last; the word itself is read only where x is inside it (x == num_docs on a word boundary: there is no such word).
__device__ __forceinline__ uint32_t filter_rank(const uint64_t* bits, const uint32_t* rank, uint32_t x) {
    const uint32_t w = x >> 6, r = x & 63u;
    return rank[w] + (r ? uint32_t(__popcll(bits[w] & ((1ull << r) - 1ull))) : 0u);
}

// Block liveness and the workgroup level of the live rank, a thread per block of the index: block b is live iff the
// filter holds a document of [base, max], clipped to the filter's num_docs. live[b] <- the flag (the host plans with
// these), out / partials as filter_word_rank_kernel's, over the flags.
__global__ __launch_bounds__(kScanThreads) void filter_block_live_kernel(const dint_block_ref* blocks, uint64_t n_blocks, const uint64_t* bits,
                                                                         const uint32_t* rank, uint32_t num_docs, uint8_t* live,
                                                                         uint32_t* out, uint32_t* partials) {
    __shared__ uint32_t wave_totals[kScanThreads / 64];
    const uint64_t b = uint64_t(blockIdx.x) * kScanThreads + threadIdx.x;
    uint32_t x = 0;
    if (b < n_blocks && num_docs != 0) {
        const uint32_t lo = blocks[b].base, hi = blocks[b].max < num_docs - 1 ? blocks[b].max : num_docs - 1;
        if (lo <= hi) x = filter_rank(bits, rank, hi + 1) != filter_rank(bits, rank, lo) ? 1u : 0u;  // (hi + 1 <= num_docs)
    }
    uint32_t total;
    const uint32_t before = workgroup_exclusive_sum(x, wave_totals, &total);
    if (b < n_blocks) {
        live[b] = uint8_t(x);
        out[b] = before;
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// ---- the query kernels ------------------------------------------------------------------------------------------------

// A filter as the query kernels see it.
struct doc_filter_view {
    const uint64_t* bits;         // ceil(num_docs / 64) words, the bits at and past num_docs zero
    uint32_t num_docs;
    const uint32_t* live_before;  // n_blocks + 1: the live blocks of the index before block b
};
// d in the filter? The bound first: no word past the bitmap is read.
__device__ __forceinline__ bool filter_holds(const doc_filter_view& f, uint32_t d) {
    return d < f.num_docs && ((f.bits[d >> 6] >> (d & 63u)) & 1ull) != 0;
}

// A ranked OR pass under a filter: term_first / term_blocks of the base describe the WHOLE list (the block-max search is
// the unfiltered call's), term_page its first page, and its pages are its live blocks only, in order (no live block: no
// page; the record still has its place in the term order).
struct ranked_or_filtered_pass {
    ranked_or_pass base;
    doc_filter_view filter;
    unsigned long long* matches;  // per query of the call: the union's documents in the filter (zero before the call's first pass)
};

// or_find through the live-rank page mapping: block position pos of record j's list lies in page
// term_page[j] + live_before[fb + pos] - live_before[fb]. Asked for a d IN THE FILTER only. The block the search finds —
// the list's first that ends at or past d — begins at or before d (base = the block before's max + 1 <= d), so d is in
// its [base, max]: the block is live and has a page. A table with other bases could name a dead block here: it holds no
// document of the filter, hence not d, and is answered without a page (its mapping would be the next live block's).
// find_posting's steps (list_block_of, find_in_page: dint_query_lookup.hpp) with the liveness test between them.
__device__ __forceinline__ posting or_find_live(const or_pass& p, const uint32_t* live_before, uint32_t j, uint32_t d) {
    const uint32_t fb = p.term_first[j], nb = p.term_blocks[j];
    const uint32_t pos = list_block_of(p.block_max, fb, nb, d);
    if (pos == nb) return {0, kAbsent};
    const uint32_t before = live_before[fb + pos];
    if (live_before[fb + pos + 1] == before) return {0, kAbsent};
    const uint64_t page = uint64_t(p.term_page[j] + (before - live_before[fb])) * kPageSlots;
    return {page, find_in_page(p.docs + page, p.blocks[fb + pos].n, d)};
}

// ranked_or_score_kernel under the filter: a workgroup per page, a thread per slot. A slot whose docID is not in the filter
// is dead before norm_lens is read or any list is probed: d < num_docs first, then one word. Invariant: for a d in the
// filter, every list's block that can hold d has d in its [base, max]; that block is therefore live and has a page, so the
// first-occurrence walk and the sum — terms in ascending term id, bm25_add from 0.0f — are ranked_or_score_kernel's,
// operation for operation. The live slots of a wave belong to one query: one add per wave.
__global__ __launch_bounds__(256) void ranked_or_filtered_score_kernel(ranked_or_filtered_pass r) {
    const ranked_or_pass& p = r.base;
    const or_pass& o = p.base;
    const uint32_t page = blockIdx.x;
    const uint32_t k = o.page_term[page];
    const uint32_t n = o.blocks[o.page_block[page]].n;
    const uint32_t slot = threadIdx.x;
    const uint64_t at = uint64_t(page) * kPageSlots + slot;
    bool alive = slot < n;
    uint32_t d = kDeadCandidate;
    if (alive) {
        d = o.docs[at];
        alive = filter_holds(r.filter, d);
    }
    float sc = 0.0f;
    if (alive) {
        const uint32_t from = o.term_from[k], n_terms = p.term_n[k];
        const float kd = bm25_kd(p.norm_lens[d]);
        for (uint32_t i = 0; i != n_terms; ++i) {
            const uint32_t j = p.term_order[from + i];
            float f;
            if (j == k) {
                f = float(o.freqs[at]);
            } else {
                const posting hit = or_find_live(o, r.filter.live_before, j, d);
                if (!hit.held()) continue;
                if (j < k) {  // an earlier list holds d: its posting there is the representative
                    alive = false;
                    break;
                }
                f = float(o.freqs[hit.slot()]);
            }
            sc = bm25_add(sc, p.term_weight[j], f, kd);
        }
    }
    p.cand[at] = alive ? d : kDeadCandidate;
    if (alive) p.score[at] = sc;
    const uint32_t n_alive = uint32_t(__popcll(__ballot(alive)));
    if ((threadIdx.x & 63u) == 0 && n_alive) atomicAdd(&r.matches[o.term_query[k]], (unsigned long long)n_alive);
}

// The filtered AND call, behind the candidates' decode and before the first round's search: a candidate not in the filter
// dies, so it never claims a block of another list. A workgroup per candidate page, a thread per slot.
__global__ __launch_bounds__(256) void filter_kill_kernel(uint32_t* cand, uint64_t n_slots, doc_filter_view f) {
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t c = cand[i];
    if (c == kDeadCandidate) return;
    if (!filter_holds(f, c)) cand[i] = kDeadCandidate;
}

}  // namespace dint_dev
