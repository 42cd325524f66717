// MaxScore-pruned ranked OR queries (the dynamic pruning of maxscore_query, reference include/ds2i/queries.hpp:459-573,
// fitted to the set-at-a-time OR pass): the same top k as ranked_or_score_kernel's pass, bit for bit, without decoding
// the blocks of the low-weight lists that no surviving candidate falls in. DESIGN.md 4d-maxscore.
//
// Per query, with the threshold theta of its seed term (the k-th best single-term addend: ranked_or_score_kernel over
// one-term records, then ranked_topk) and the host's split of its terms into the essential ones E and the rest N:
//   1. ms_bound_kernel: a thread per posting of E's decoded pages. A posting is its document's representative iff no E
//      list before its own (longest first) holds it. The representative sums its E addends in double (P, in E's order)
//      and dies if (P + sum_N m_t) * margin < theta; a live one claims, for every N term whose pages are not decoded,
//      the block its docID falls in (block-max search). Claims are per (term record, block): a flag, a rank, a touched list.
//   2. The host decodes the claimed blocks behind the other pages (docs and freqs).
//   3. ms_score_kernel: every live representative walks ALL of the query's terms in ascending term id and adds
//      q_weight * f / (f + kd) from 0.0f, binary32, uncontracted — ranked_or_score_kernel's operations in its order —
//      probing decoded terms through their pages and N terms through their claimed blocks.
// ranked_topk then selects over the candidate pages. Nothing is added atomically but the claim counters.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_query_kernels.hpp"
#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

// One pass of a pruned call, after its seeds: every distinct term of every query is a term record (a query's records
// consecutive, longest list first); the decoded pages (seeds, then the other E terms, then the claimed blocks) in docs /
// freqs; the candidate pages (E's pages, query after query) map onto them.
struct maxscore_pass {
    const uint32_t* term_first;    // record -> first block of its list in the index
    const uint32_t* term_blocks;   // ... its list's block count
    const uint32_t* term_page;     // ... decoded: its first page in docs; claimed (N): its first claim flag
    const uint32_t* term_claimed;  // ... 1: an N term probed through its claimed blocks
    const float* term_weight;      // ... q_weight of its term in its query
    const uint32_t* term_order;    // [q_from[q] + i] = the record of query q's i-th smallest term id
    const uint32_t* term_e;        // [q_from[q] + i], i < q_ne[q]: query q's E records, longest first
    const uint32_t* q_from;        // pass query -> its first record
    const uint32_t* q_n;           // ... its records
    const uint32_t* q_ne;          // ... its E records
    const float* q_theta;          // ... theta (0: nothing is pruned)
    const double* q_rest;          // ... sum over N of (double) m_t, in N's order
    const double* q_margin;        // ... 1 + (|T| + 1) * 2^-23
    const uint32_t* cpage_page;    // candidate page -> its page in docs
    const uint32_t* cpage_rec;     // ... its term record (an E term)
    const uint32_t* rec_query;     // record -> pass query
    const dint_block_ref* blocks;
    const uint32_t* block_max;
    const uint32_t* docs;
    const uint32_t* freqs;
    uint32_t claim_page0;          // the first page of the claimed blocks in docs
    uint32_t* flag;                // per claim flag: 1 once claimed (zero at launch)
    uint32_t* rank;                // ... its place in touched
    uint32_t* touched;             // the claimed blocks, by index block id
    uint32_t* n_touched;
    uint32_t* q_claims;            // pass query -> the blocks it claimed
    const float* norm_lens;
    uint32_t* cand;                // per candidate slot: the representative's docID, kDeadCandidate otherwise
    float* score;
};

// d in the decoded page of record j? -> its position there, or ~0u
__device__ __forceinline__ uint32_t ms_find_decoded(const maxscore_pass& p, uint32_t j, uint32_t d, uint64_t& pg) {
    const uint32_t fb = p.term_first[j], nb = p.term_blocks[j];
    const uint32_t pos = lower_bound_u32(p.block_max + fb, nb, d);
    if (pos == nb) return ~0u;  // past the list's last docID
    const uint32_t m = p.blocks[fb + pos].n;
    pg = uint64_t(p.term_page[j] + pos) * kPageSlots;
    const uint32_t hit = lower_bound_u32(p.docs + pg, m, d);
    return hit != m && p.docs[pg + hit] == d ? hit : ~0u;
}

// A workgroup per candidate page, a thread per slot. The loops over a query's records are uniform in the workgroup (a
// page is one query's), so the wave-neighbour test of the claims sees every lane.
__global__ __launch_bounds__(256) void ms_bound_kernel(maxscore_pass p) {
#pragma clang fp contract(off)
    const uint32_t cp = blockIdx.x;
    const uint32_t page = p.cpage_page[cp], k = p.cpage_rec[cp];
    const uint32_t q = p.rec_query[k];
    const uint32_t n = p.blocks[p.term_first[k] + (page - p.term_page[k])].n;
    const uint32_t slot = threadIdx.x;
    const uint64_t at = uint64_t(page) * kPageSlots + slot, c_at = uint64_t(cp) * kPageSlots + slot;
    bool alive = slot < n;
    const uint32_t d = alive ? p.docs[at] : kDeadCandidate;
    if (alive) {
        const float kd = kBm25K1 * ((1.0f - kBm25B) + kBm25B * p.norm_lens[d]);
        const uint32_t from = p.q_from[q], ne = p.q_ne[q];
        bool before = true;  // (still in the E lists before this one)
        double P = 0.0;
        for (uint32_t i = 0; i != ne && alive; ++i) {
            const uint32_t j = p.term_e[from + i];
            float f;
            if (j == k) {
                before = false;
                f = float(p.freqs[at]);
            } else {
                uint64_t pg = 0;
                const uint32_t hit = ms_find_decoded(p, j, d, pg);
                if (hit == ~0u) continue;
                if (before) {  // an earlier E list holds d: its posting there is the representative
                    alive = false;
                    break;
                }
                f = float(p.freqs[pg + hit]);
            }
            const float w = f / (f + kd);
            const float a = p.term_weight[j] * w;
            P = P + double(a);
        }
        if (alive && (P + p.q_rest[q]) * p.q_margin[q] < double(p.q_theta[q])) alive = false;  // strict: a tie with theta stays
    }
    p.cand[c_at] = alive ? d : kDeadCandidate;
    // claims: per N term whose pages are not decoded, the block of every live candidate (neighbours in a wave share one)
    const uint32_t from = p.q_from[q], nr = p.q_n[q];
    for (uint32_t j = from; j != from + nr; ++j) {
        if (!p.term_claimed[j]) continue;
        uint32_t idx = kDeadCandidate;
        if (alive) {
            const uint32_t fb = p.term_first[j], nb = p.term_blocks[j];
            const uint32_t pos = lower_bound_u32(p.block_max + fb, nb, d);
            if (pos != nb) idx = p.term_page[j] + pos;
        }
        const uint32_t prev = __shfl_up(idx, 1);
        const bool lead = idx != kDeadCandidate && ((threadIdx.x & 63u) == 0 || prev != idx);
        if (lead && atomicExch(&p.flag[idx], 1u) == 0u) {
            const uint32_t r = atomicAdd(p.n_touched, 1u);
            p.touched[r] = p.term_first[j] + (idx - p.term_page[j]);
            p.rank[idx] = r;
            atomicAdd(&p.q_claims[q], 1u);
        }
    }
}

// A workgroup per candidate page, a thread per live representative: its whole score, as ranked_or_score_kernel sums it.
__global__ __launch_bounds__(256) void ms_score_kernel(maxscore_pass p) {
#pragma clang fp contract(off)
    const uint32_t cp = blockIdx.x;
    const uint64_t c_at = uint64_t(cp) * kPageSlots + threadIdx.x;
    const uint32_t d = p.cand[c_at];
    if (d == kDeadCandidate) return;
    const uint32_t page = p.cpage_page[cp], k = p.cpage_rec[cp];
    const uint32_t q = p.rec_query[k];
    const uint64_t at = uint64_t(page) * kPageSlots + threadIdx.x;
    const uint32_t from = p.q_from[q], nr = p.q_n[q];
    const float kd = kBm25K1 * ((1.0f - kBm25B) + kBm25B * p.norm_lens[d]);
    float sc = 0.0f;
    for (uint32_t i = 0; i != nr; ++i) {
        const uint32_t j = p.term_order[from + i];
        float f;
        if (j == k) {
            f = float(p.freqs[at]);
        } else if (!p.term_claimed[j]) {
            uint64_t pg = 0;
            const uint32_t hit = ms_find_decoded(p, j, d, pg);
            if (hit == ~0u) continue;
            f = float(p.freqs[pg + hit]);
        } else {  // (this candidate claimed the block: its rank is set)
            const uint32_t fb = p.term_first[j], nb = p.term_blocks[j];
            const uint32_t pos = lower_bound_u32(p.block_max + fb, nb, d);
            if (pos == nb) continue;
            const uint32_t m = p.blocks[fb + pos].n;
            const uint64_t pg = uint64_t(p.claim_page0 + p.rank[p.term_page[j] + pos]) * kPageSlots;
            const uint32_t hit = lower_bound_u32(p.docs + pg, m, d);
            if (hit == m || p.docs[pg + hit] != d) continue;
            f = float(p.freqs[pg + hit]);
        }
        const float w = f / (f + kd);
        sc = sc + p.term_weight[j] * w;
    }
    p.score[c_at] = sc;
}

}  // namespace dint_dev
