// Ranked disjunctive queries (ranked_or_query, reference include/ds2i/queries.hpp:387-457): BM25 scores of every document
// of a query's union, for the per-query top-k of the ranked selection (dint_ranked_query_kernels.hpp).
//
// A pass is an OR pass (dint_or_query_kernels.hpp): whole queries, the distinct terms of each longest list first, every
// block of every term decoded with its freqs. A posting d of the k-th list is its union's representative iff no earlier
// list holds d (the first occurrence of or_count_kernel); the representative alone computes d's whole score, so a
// document is scored by exactly one thread and nothing is added atomically. It walks the query's terms in ascending term
// id — the order query_freqs (queries.hpp:135-148) hands ranked_or_query its cursors in, and so the order its sum runs
// in — and adds the BM25 addend (bm25_add) of every term whose list holds d, from 0.0f. A term is its own list (its freq is
// the slot's own) or is probed once (or_find; DESIGN.md 4d, "Shared device primitives"). A hit in a list before its own
// (longer, or as long with a smaller term id) kills the slot: the walk decides that on its way.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_or_query_kernels.hpp"
#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

// An OR pass with what a ranked one reads besides: per term record, the records of its query in term-id order and the
// query's term weight; per slot, where the candidate and its score go.
struct ranked_or_pass {
    or_pass base;                 // (freqs: never null; counts / freq_sums: unused)
    const uint32_t* term_order;   // [term_from[k] + i] = the record of the i-th smallest term id of record k's query
    const uint32_t* term_n;       // term record -> distinct terms of its query
    const float* term_weight;     // term record -> q_weight of its term in its query
    const float* norm_lens;       // the wand handle's, by docID
    uint32_t* cand;               // per pass slot: the docID of a representative, kDeadCandidate otherwise
    float* score;                 // per pass slot: the representative's score
};

// A workgroup per page (256 slots), a thread per slot, as or_count_kernel. The slots past the block's n are padding: dead.
__global__ __launch_bounds__(256) void ranked_or_score_kernel(ranked_or_pass p) {
    const or_pass& o = p.base;
    const uint32_t page = blockIdx.x;
    const uint32_t k = o.page_term[page];
    const uint32_t n = o.blocks[o.page_block[page]].n;
    const uint32_t slot = threadIdx.x;
    const uint64_t at = uint64_t(page) * kPageSlots + slot;
    if (slot >= n) {
        p.cand[at] = kDeadCandidate;
        return;
    }
    const uint32_t d = o.docs[at];
    const uint32_t from = o.term_from[k], n_terms = p.term_n[k];
    const float kd = bm25_kd(p.norm_lens[d]);
    float sc = 0.0f;
    for (uint32_t i = 0; i != n_terms; ++i) {
        const uint32_t j = p.term_order[from + i];
        float f;
        if (j == k) {
            f = float(o.freqs[at]);
        } else {
            const posting hit = or_find(o, j, d);
            if (!hit.held()) continue;
            if (j < k) {  // an earlier list holds d: its posting there is the representative
                p.cand[at] = kDeadCandidate;
                return;
            }
            f = float(o.freqs[hit.slot()]);
        }
        sc = bm25_add(sc, p.term_weight[j], f, kd);
    }
    p.cand[at] = d;
    p.score[at] = sc;
}

}  // namespace dint_dev
