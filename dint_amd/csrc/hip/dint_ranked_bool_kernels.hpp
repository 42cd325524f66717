// Ranked boolean queries (required, optional and excluded terms — ranked_and_query, reference
// include/ds2i/queries.hpp:309-385, generalised; the cursor primitive is next_geq + freq(),
// include/dint/dict_posting_list.hpp:126-169): the per-term steps that run behind the AND rounds over the survivors in
// their candidate slots. Unlike the freqs pass of the required terms (and_freq_search_kernel: "a match: always found"), a
// live candidate need not be in the step's list:
//   search   bool_search_kernel: the block of the step's term the candidate can be in, claimed once; none past the list's end
//   exclude  bool_exclude_kernel: a candidate found in the decoded docs part of its block is killed
//   optional bool_should_gather_kernel: a candidate found adds its term's BM25 addend to its slot; one not found is left alone
// A thread per candidate slot, a launch per term step, as ranked_gather_kernel: no atomics on scores, no float reductions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

// The step's search: term_first / term_blocks give, per query, the block range of the step's list (term_blocks == 0: the
// query has no term at this step, or an empty list — its candidates claim nothing). target[i] <- the block (kDeadCandidate:
// none — no term, or the candidate lies past the list's last docID), claimed once per block, as in and_search_kernel.
// (gb is kDeadCandidate on every path that claims nothing, so the whole wave reaches run_leader's shuffle.)
__global__ void bool_search_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, const uint32_t* term_first,
                                   const uint32_t* term_blocks, const uint32_t* block_max, uint32_t* target, uint32_t* needed,
                                   uint32_t* rank, uint32_t* touched, uint32_t* n_touched) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    uint32_t gb = kDeadCandidate;
    if (i < n_slots) {
        const uint32_t c = cand[i];
        if (c != kDeadCandidate) {
            const uint32_t q = page_query[i / kPageSlots];
            const uint32_t nb = term_blocks[q];
            if (nb) {
                const uint32_t fb = term_first[q];
                const uint32_t pos = list_block_of(block_max, fb, nb, c);
                if (pos != nb) gb = fb + pos;  // (pos == nb: next_geq past the last block — not in the list)
            }
            target[i] = gb;
        }
    }
    if (run_leader(gb)) claim_dense(needed, rank, touched, n_touched, gb, gb);
}

// The position of live candidate i's docID in the decoded page of its target block -> the slot in probe / fprobe, or
// kAbsent (a dead slot, no target, or the docID is not in the block).
struct bool_hit {
    uint64_t slot;
    bool held;
};
__device__ __forceinline__ bool_hit bool_find(const uint32_t* cand, uint64_t i, const dint_block_ref* blocks, const uint32_t* target,
                                              const uint32_t* rank, const uint32_t* probe) {
    const uint32_t c = cand[i];
    if (c == kDeadCandidate) return {0, false};
    const uint32_t gb = target[i];
    if (gb == kDeadCandidate) return {0, false};
    const uint32_t n = blocks[gb].n;
    const uint64_t page = uint64_t(rank[gb]) * kPageSlots;
    const uint32_t pos = find_in_page(probe + page, n, c);
    return {page + pos, pos != kAbsent};
}

// An excluded term: the candidate is in the list -> no match.
__global__ void bool_exclude_kernel(uint32_t* cand, uint64_t n_slots, const dint_block_ref* blocks, const uint32_t* target,
                                    const uint32_t* rank, const uint32_t* probe) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    if (bool_find(cand, i, blocks, target, rank, probe).held) cand[i] = kDeadCandidate;
}

// An optional term: the match is in the list -> its addend, on top of the required terms' sum (kden[i]: written by the
// rarest required term's gather, ranked_gather_kernel).
__global__ void bool_should_gather_kernel(const uint32_t* cand, uint64_t n_slots, const uint32_t* page_query, const dint_block_ref* blocks,
                                          const uint32_t* target, const uint32_t* rank, const uint32_t* probe, const uint32_t* fprobe,
                                          const float* q_weight, const float* kden, float* score) {
    const uint64_t i = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_slots) return;
    const bool_hit h = bool_find(cand, i, blocks, target, rank, probe);
    if (!h.held) return;
    score[i] = bm25_add(score[i], q_weight[page_query[i / kPageSlots]], float(fprobe[h.slot]), kden[i]);
}

}  // namespace dint_dev
