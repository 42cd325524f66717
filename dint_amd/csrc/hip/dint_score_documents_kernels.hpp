// BM25 scores of caller-given documents (dint_score_documents): the cursor primitive every query of the reference is built
// on — document_enumerator::next_geq(d), then freq() (include/dint/dict_posting_list.hpp:126-169) — for a batch of (query,
// document set) pairs, with ranked_or_query's sums (include/ds2i/queries.hpp:387-457). DESIGN.md 4d-score.
//
// It is MaxScore's step 5 (dint_ranked_or_maxscore_kernels.hpp) with every term probed through claimed blocks and the
// candidates handed in: no seed, no threshold, no bound, no selection.
//   1. sd_claim_kernel: a thread per (document, term record) finds the block the docID falls in (the first block whose last
//      docID is >= it: block-max search) and claims it, once per (term record, block): a flag, a rank, a touched list.
//   2. The host decodes the touched blocks' docs and freqs parts, launches sized by its own bound.
//   3. sd_score_kernel: a thread per document walks the query's terms in ascending term id and adds their addends from
//      0.0f (bm25_add) — ranked_or_score_kernel's operations in its order.
// Nothing is added atomically but the touched counter.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_query_kernels.hpp"
#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

// One pass of a call: whole queries; every distinct term of every query is a term record (a query's records consecutive),
// the pass's documents lie query after query.
struct score_documents_pass {
    const uint32_t* term_first;   // record -> first block of its list in the index
    const uint32_t* term_blocks;  // ... its list's block count
    const uint32_t* term_flag;    // ... its first claim flag (one per block of its list)
    const float* term_weight;     // ... q_weight of its term in its query
    const uint32_t* term_order;   // [q_from[q] + i] = the record of query q's i-th smallest term id
    const uint32_t* q_from;       // pass query -> its first record
    const uint32_t* q_n;          // ... its records (distinct terms)
    const uint64_t* q_freq_at;    // ... where its freqs matrix begins in freqs_out, less its first document's row
    const uint32_t* doc_query;    // pass document -> pass query
    const uint32_t* doc_id;       // ... its docID (any u32)
    uint32_t n_docs;
    const dint_block_ref* blocks;
    const uint32_t* block_max;
    const uint32_t* docs;         // the touched blocks' pages, in touched order
    const uint32_t* freqs;
    uint32_t* flag;               // per claim flag: 1 once claimed (zero at launch)
    uint32_t* rank;               // ... its place in touched
    uint32_t* touched;            // the claimed blocks, by index block id
    uint32_t* n_touched;          // (zero at launch; the pass's blocks read)
    const float* norm_lens;
    float* score_out;             // per pass document
    uint32_t* freqs_out;          // null: not wanted
};

// grid.x over the pass's documents, grid.y over the term ranks (a query with fewer terms leaves the others idle).
// Neighbours in a wave that fall into one block share its claim.
__global__ __launch_bounds__(256) void sd_claim_kernel(score_documents_pass p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < p.n_docs;
    const uint32_t q = in ? p.doc_query[i] : 0u;
    const uint32_t d = in ? p.doc_id[i] : 0u;
    const uint32_t from = in ? p.q_from[q] : 0u, nr = in ? p.q_n[q] : 0u;
    // (the loop is bounded by the launch, not by the thread: the wave-neighbour test below needs every lane)
    for (uint32_t r = blockIdx.y; __any(r < nr); r += gridDim.y) {
        uint32_t idx = kDeadCandidate, gb = 0;
        if (r < nr) {
            const uint32_t j = from + r;
            const uint32_t fb = p.term_first[j], nb = p.term_blocks[j];
            const uint32_t pos = list_block_of(p.block_max, fb, nb, d);
            if (pos != nb) {  // (a document past the list's last docID claims nothing)
                idx = p.term_flag[j] + pos;
                gb = fb + pos;
            }
        }
        if (run_leader(idx)) claim_dense(p.flag, p.rank, p.touched, p.n_touched, idx, gb);
    }
}

// A thread per document: its whole score, as ranked_or_score_kernel sums it, and its row of freqs.
__global__ __launch_bounds__(256) void sd_score_kernel(score_documents_pass p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.n_docs) return;
    const uint32_t q = p.doc_query[i], d = p.doc_id[i];
    const uint32_t from = p.q_from[q], nr = p.q_n[q];
    uint32_t* const row = p.freqs_out ? p.freqs_out + (p.q_freq_at[q] + uint64_t(i) * nr) : nullptr;
    bool have_kd = false;  // (norm_lens[d] exists once some list holds d: d may be any u32)
    float kd = 0.0f;
    float sc = 0.0f;
    for (uint32_t r = 0; r != nr; ++r) {
        const uint32_t j = p.term_order[from + r];
        // (this document claimed the block its docID falls in: its rank is set)
        const posting hit = find_posting(p.block_max, p.blocks, p.term_first[j], p.term_blocks[j], p.docs, d,
                                         [&](uint32_t pos) { return p.rank[p.term_flag[j] + pos]; });
        const uint32_t fr = hit.held() ? p.freqs[hit.slot()] : 0u;
        if (row) row[r] = fr;
        if (!hit.held()) continue;
        if (!have_kd) {
            kd = bm25_kd(p.norm_lens[d]);
            have_kd = true;
        }
        sc = bm25_add(sc, p.term_weight[j], float(fr), kd);
    }
    p.score_out[i] = sc;
}

}  // namespace dint_dev
