// Disjunctive (OR) queries over the in-index layout, batched: the set-at-a-time form of or_query<with_freqs>
// (reference include/ds2i/queries.hpp:86-130), which visits every docID some list of the query holds, once.
//
// "First occurrence": order a query's distinct terms t_0 .. t_{T-1} (longest list first). A posting d of t_k is counted
// iff d is in none of t_0 .. t_{k-1}, so
//     count(q) = sum_k #{d in L_k : d not in L_j for all j < k}
// and every docID of the union is counted exactly once, at the first list that holds it. Every block of every term is
// decoded into pages (decode_pages), the query's pages term after term; then ONE launch, a workgroup per page, a thread
// per slot, probes each posting against the lists before its own (find_posting: DESIGN.md 4d, "Shared device primitives").
// The pages are only read: nothing is retired the way the AND probe retires its candidates.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_hip.h"
#include "dint_query_kernels.hpp"

namespace dint_dev {

// One pass of an OR call: whole queries, their terms' pages decoded into docs (and freqs) at term_page[k] onwards.
struct or_pass {
    const uint32_t* page_block;   // pass page -> block of the index
    const uint32_t* page_term;    // pass page -> term record
    const uint32_t* term_first;   // term record -> first block of its list in the index
    const uint32_t* term_blocks;  // ... its list's block count (= its pages)
    const uint32_t* term_page;    // ... its first page in the pass
    const uint32_t* term_query;   // ... its query (in the call)
    const uint32_t* term_from;    // ... the record of its query's first (longest) term
    const dint_block_ref* blocks;
    const uint32_t* block_max;
    const uint32_t* docs;         // the pass's pages, kPageSlots slots each
    const uint32_t* freqs;        // null: no freqs
    unsigned long long* counts;   // per query of the call
    unsigned long long* freq_sums;
};

// d in the list of term record j, every block of which lies decoded from page term_page[j] on? -> where
__device__ __forceinline__ posting or_find(const or_pass& p, uint32_t j, uint32_t d) {
    return find_posting(p.block_max, p.blocks, p.term_first[j], p.term_blocks[j], p.docs, d,
                        [&](uint32_t pos) { return p.term_page[j] + pos; });
}

// A workgroup per page (256 slots = 4 waves), a thread per slot. A page is one term's block of one query, so a wave's
// survivors all belong to one query: one atomic per wave. The slots past the block's n are padding and never count.
__global__ __launch_bounds__(256) void or_count_kernel(or_pass p) {
    const uint32_t page = blockIdx.x;
    const uint32_t k = p.page_term[page];
    const uint32_t q = p.term_query[k];
    const uint32_t n = p.blocks[p.page_block[page]].n;
    const uint32_t slot = threadIdx.x;
    bool alive = slot < n;
    uint32_t f = 0;
    if (alive) {
        const uint64_t at = uint64_t(page) * kPageSlots + slot;
        const uint32_t d = p.docs[at];
        if (p.freqs) f = p.freqs[at];
        for (uint32_t j = p.term_from[k]; j != k; ++j) {  // the lists before this one: does one of them hold d?
            if (or_find(p, j, d).held()) {
                alive = false;
                break;
            }
        }
    }
    const uint32_t n_alive = uint32_t(__popcll(__ballot(alive)));
    unsigned long long fs = f;
    if (p.freqs)  // (uniform)
        for (int off = 32; off != 0; off >>= 1) fs += __shfl_xor(fs, off);
    if ((threadIdx.x & 63u) != 0) return;
    if (n_alive) atomicAdd(&p.counts[q], (unsigned long long)n_alive);
    if (p.freqs && fs) atomicAdd(&p.freq_sums[q], fs);
}

}  // namespace dint_dev
