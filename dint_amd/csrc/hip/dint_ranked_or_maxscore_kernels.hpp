// MaxScore-pruned ranked OR queries (the dynamic pruning of maxscore_query, reference include/ds2i/queries.hpp:459-573,
// fitted to the set-at-a-time OR pass): the same top k as ranked_or_score_kernel's pass, bit for bit, without decoding
// the blocks of the low-weight lists that no surviving candidate falls in. DESIGN.md 4d-maxscore.
//
// Per query, with the threshold theta of its seed term (the k-th best single-term addend: ranked_or_score_kernel over
// one-term records, then ranked_topk) and the host's split of its terms into the essential ones E and the rest N:
//   1. ms_bound_kernel: a thread per posting of E's decoded pages. A posting is its document's representative iff no E
//      list before its own (longest first) holds it. The representative sums its E addends in double (P, in E's order)
//      and dies if (P + sum_N m_t) * margin < theta — with block maxima, also if the candidate's own sum over N does it:
//      per N term, q_weight * the maximum of the block its docID falls in (ms_block_rest) — a live one claims, for every N term whose pages are not decoded,
//      the block its docID falls in (block-max search). Claims are per (term record, block): a flag, a rank, a touched list.
//   2. The host decodes the claimed blocks behind the other pages (docs and freqs).
//   3. ms_score_kernel: every live representative walks ALL of the query's terms in ascending term id and adds their
//      addends from 0.0f (bm25_add) — ranked_or_score_kernel's operations in its order — probing decoded terms through
//      their pages and N terms through their claimed blocks.
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
    const uint32_t* term_claimed;  // ... 0: an E term; 1: an N term probed through its claimed blocks; 2: a seed in N (its pages are decoded)
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
    const float* block_max_weight; // nullable; per index block: the largest doc_term_weight of its postings (block maxima)
    uint32_t* cand;                // per candidate slot: the representative's docID, kDeadCandidate otherwise
    float* score;
};

// d in the list of record j? -> where. A decoded record's blocks lie from page term_page[j] on; a claimed one's block
// is at its rank behind claim_page0 (asked by a candidate that claimed it).
__device__ __forceinline__ posting ms_find(const maxscore_pass& p, uint32_t j, uint32_t d, bool claimed) {
    return find_posting(p.block_max, p.blocks, p.term_first[j], p.term_blocks[j], p.docs, d, [&](uint32_t pos) {
        return claimed ? p.claim_page0 + p.rank[p.term_page[j] + pos] : p.term_page[j] + pos;
    });
}

// Block maxima: what the N terms can still add to document d of query q. From 0.0, over the N terms in ascending term id,
// (double) fl32(q_weight_t * block_max_weight[b_t(d)]), b_t(d) the block of t that d falls in (the claims' lookup); a
// term whose list ends before d adds nothing. fl32(q_w * maximum) >= every addend of that block (rounding is monotone).
__device__ __forceinline__ double ms_block_rest(const maxscore_pass& p, uint32_t q, uint32_t d) {
#pragma clang fp contract(off)
    const uint32_t from = p.q_from[q], nr = p.q_n[q];
    double rest = 0.0;
    for (uint32_t i = 0; i != nr; ++i) {
        const uint32_t j = p.term_order[from + i];
        if (!p.term_claimed[j]) continue;
        const uint32_t nb = p.term_blocks[j];
        const uint32_t pos = list_block_of(p.block_max, p.term_first[j], nb, d);
        if (pos == nb) continue;
        const float m = p.term_weight[j] * p.block_max_weight[p.term_first[j] + pos];
        rest = rest + double(m);
    }
    return rest;
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
        const float kd = bm25_kd(p.norm_lens[d]);
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
                const posting hit = ms_find(p, j, d, false);
                if (!hit.held()) continue;
                if (before) {  // an earlier E list holds d: its posting there is the representative
                    alive = false;
                    break;
                }
                f = float(p.freqs[hit.slot()]);
            }
            P = P + double(bm25_addend(p.term_weight[j], f, kd));
        }
        if (alive) {
            double rest = p.q_rest[q];
            if (p.block_max_weight) {  // (the smaller of the two bounds: block maxima above their term's maximum cost nothing)
                const double by_block = ms_block_rest(p, q, d);
                rest = by_block < rest ? by_block : rest;
            }
            if ((P + rest) * p.q_margin[q] < double(p.q_theta[q])) alive = false;  // strict: a tie with theta stays
        }
    }
    p.cand[c_at] = alive ? d : kDeadCandidate;
    // claims: per N term whose pages are not decoded, the block of every live candidate (neighbours in a wave share one)
    const uint32_t from = p.q_from[q], nr = p.q_n[q];
    for (uint32_t j = from; j != from + nr; ++j) {
        if (p.term_claimed[j] != 1) continue;
        uint32_t idx = kDeadCandidate;
        if (alive) {
            const uint32_t nb = p.term_blocks[j];
            const uint32_t pos = list_block_of(p.block_max, p.term_first[j], nb, d);
            if (pos != nb) idx = p.term_page[j] + pos;
        }
        if (run_leader(idx) && claim_dense(p.flag, p.rank, p.touched, p.n_touched, idx, p.term_first[j] + (idx - p.term_page[j])))
            atomicAdd(&p.q_claims[q], 1u);
    }
}

// A workgroup per candidate page, a thread per live representative: its whole score, as ranked_or_score_kernel sums it.
__global__ __launch_bounds__(256) void ms_score_kernel(maxscore_pass p) {
    const uint32_t cp = blockIdx.x;
    const uint64_t c_at = uint64_t(cp) * kPageSlots + threadIdx.x;
    const uint32_t d = p.cand[c_at];
    if (d == kDeadCandidate) return;
    const uint32_t page = p.cpage_page[cp], k = p.cpage_rec[cp];
    const uint32_t q = p.rec_query[k];
    const uint64_t at = uint64_t(page) * kPageSlots + threadIdx.x;
    const uint32_t from = p.q_from[q], nr = p.q_n[q];
    const float kd = bm25_kd(p.norm_lens[d]);
    float sc = 0.0f;
    for (uint32_t i = 0; i != nr; ++i) {
        const uint32_t j = p.term_order[from + i];
        float f;
        if (j == k) {
            f = float(p.freqs[at]);
        } else {
            const posting hit = ms_find(p, j, d, p.term_claimed[j] == 1);
            if (!hit.held()) continue;
            f = float(p.freqs[hit.slot()]);
        }
        sc = bm25_add(sc, p.term_weight[j], f, kd);
    }
    p.score[c_at] = sc;
}

}  // namespace dint_dev
