// Union-driven ranked boolean queries (optional terms with a minimum number that must match, less excluded terms — Lucene's
// pure SHOULD with MUST_NOT and minimum_should_match; ranked_or_query, reference include/ds2i/queries.hpp:387-457, with
// next_geq, include/dint/dict_posting_list.hpp:126-169, for the exclusions): the scoring launch of an OR pass that also
// counts the lists a document is in.
//
// The pass, the first-occurrence rule and the walk are ranked_or_score_kernel's (dint_ranked_or_query_kernels.hpp): the
// representative of a document d walks its query's terms in ascending term id, finds d's posting in every other list
// (or_find) and adds bm25_add of the lists that hold d, from 0.0f — so a survivor's score is dint_ranked_or_queries', bit
// for bit. On its way it counts those lists, its own among them; a representative in fewer than its query's m lists is no
// match: kDeadCandidate, like a slot that is no representative. The excluded terms then run over the same slots with the
// steps of the ranked boolean call (bool_search_kernel, bool_exclude_kernel: dint_ranked_bool_kernels.hpp); no kernel of
// its own, and no search of its own here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_ranked_or_query_kernels.hpp"

namespace dint_dev {

// A ranked OR pass and, per term record, its query's m (>= 1: the distinct optional terms whose list must hold a match).
struct ranked_or_bool_pass {
    ranked_or_pass base;
    const uint32_t* term_m;
};

// A workgroup per page, a thread per slot, as ranked_or_score_kernel. The walk ends early once the lists found and the
// terms still to come cannot reach m: the slot is dead either way (a later hit in an earlier list would only kill it too).
__global__ __launch_bounds__(256) void ranked_or_bool_score_kernel(ranked_or_bool_pass b) {
#pragma clang fp contract(off)  // (the sums are bm25_add's, which carries its own: nothing here may become an fma either)
    const ranked_or_pass& p = b.base;
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
    const uint32_t from = o.term_from[k], n_terms = p.term_n[k], m = b.term_m[k];
    const float kd = bm25_kd(p.norm_lens[d]);
    float sc = 0.0f;
    uint32_t held = 0;
    for (uint32_t i = 0; i != n_terms; ++i) {
        if (held + (n_terms - i) < m) break;  // (held < m from here on: dead below)
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
        held += 1;
        sc = bm25_add(sc, p.term_weight[j], f, kd);
    }
    if (held < m) {
        p.cand[at] = kDeadCandidate;
        return;
    }
    p.cand[at] = d;
    p.score[at] = sc;
}

}  // namespace dint_dev
