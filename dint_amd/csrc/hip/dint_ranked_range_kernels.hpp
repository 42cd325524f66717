// DocID-range ranked queries: the ranked OR and ranked AND calls restricted, per query, to the documents of a half-open
// docID interval [lo, hi). The range is a filter — a match scores exactly what the unranged call gives
// it — and a skipping feature: the host plans only the blocks that can hold a docID of the range (list_blocks_in_range,
// dint_query_lookup.hpp), so these kernels see restricted page sets. What is left for them is the boundary: the first and
// the last block of a restricted set may hold docIDs outside the range, and those slots die here before they cost anything.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_ranked_or_query_kernels.hpp"

namespace dint_dev {

// A ranked OR pass whose term records are restricted to their query's range: term_first / term_blocks / term_page of the
// base describe only the list's blocks in range (0 blocks: none, the record still has its place in the term order).
struct ranked_or_range_pass {
    ranked_or_pass base;
    const uint32_t* term_lo;      // term record -> its query's range, [lo, hi)
    const uint32_t* term_hi;
    unsigned long long* matches;  // per query of the call: the union's documents in range (zero before the call's first pass)
};

// ranked_or_score_kernel with the range: a workgroup per page, a thread per slot. A slot whose docID is outside [lo, hi) is
// dead before norm_lens is read or any list is probed. For a docID in range, the block of any list that can hold it is in
// that list's restricted set, so the first-occurrence walk and the sum — terms in ascending term id, bm25_add from 0.0f —
// are ranked_or_score_kernel's, operation for operation. The live slots of a wave belong to one query: one add per wave.
__global__ __launch_bounds__(256) void ranked_or_range_score_kernel(ranked_or_range_pass r) {
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
        alive = d >= r.term_lo[k] && d < r.term_hi[k];
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
                const posting hit = or_find(o, j, d);
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

// The ranged AND call, behind the candidates' decode and before the first round's search: a candidate outside its query's
// range dies, so it never claims a block of another list. q_range: per query {lo, hi}. A workgroup per candidate page.
__global__ __launch_bounds__(256) void range_kill_kernel(uint32_t* cand, uint64_t n_slots, const uint32_t* page_query,
                                                         const uint32_t* q_range) {
    const uint64_t i = uint64_t(blockIdx.x) * kPageSlots + threadIdx.x;
    if (i >= n_slots) return;
    const uint32_t c = cand[i];
    if (c == kDeadCandidate) return;
    const uint32_t q = page_query[blockIdx.x];
    if (c < q_range[2 * q] || c >= q_range[2 * q + 1]) cand[i] = kDeadCandidate;
}

}  // namespace dint_dev
