// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": union-driven ranked boolean
// queries — optional terms of which at least m must occur, less excluded terms (ranked_or_query, queries.hpp:387-457, with
// next_geq, dict_posting_list.hpp:126-169, for the exclusions: DESIGN.md 4d-or-bool).
// ---- union-driven ranked boolean queries ----------------------------------------------------------
// The call is a ranked OR call (or_queries_impl with rk) over the optional terms, with or_bool_args hooked into its passes:
//   1 the pass's pages decoded, docs and freqs (eager: every block of every distinct optional term)
//   2 ranked_or_bool_score_kernel: the union's representatives scored as ranked_or_score_kernel scores them; the ones in
//     fewer than m lists are dropped
//   3 per excluded term, in ascending term id: bool_step over the pass's slots (lazy: docs parts only, of the blocks a
//     survivor falls in)
//   4 and_count_kernel: the matches, 5 ranked_topk, and with the last pass the counters' copy back
// A query that cannot match — no blocks, or m above its distinct terms — is in no pass (plan_or_passes).

int dint_ranked_or_bool_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                const uint32_t* should_terms, const uint64_t* should_offsets, const uint32_t* not_terms,
                                const uint64_t* not_offsets, const uint32_t* min_should_match, size_t n_queries, uint64_t* counts,
                                uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, should_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    const bool_clause should{should_terms, should_offsets}, exclude{not_terms, not_offsets};
    if (!should.ok(qi, n_queries) || !exclude.ok(qi, n_queries)) return DINT_ERR_ARG;
    if (blocks_decoded) *blocks_decoded = 0;
    if (n_queries == 0) return DINT_OK;

    or_bool_args x;
    std::vector<uint32_t> m(n_queries, 1u);
    if (min_should_match)
        for (size_t q = 0; q != n_queries; ++q) m[q] = std::max<uint32_t>(1u, min_should_match[q]);
    x.m = m.data();
    x.not_at.assign(n_queries + 1, 0);
    if (not_offsets) {  // every query's excluded terms, distinct and ascending, in one flat copy
        x.not_terms.reserve(size_t(not_offsets[n_queries] - not_offsets[0]));
        for (size_t q = 0; q != n_queries; ++q) {
            const size_t from = x.not_terms.size();
            x.not_terms.insert(x.not_terms.end(), not_terms + not_offsets[q], not_terms + not_offsets[q + 1]);
            std::sort(x.not_terms.begin() + from, x.not_terms.end());
            x.not_terms.erase(std::unique(x.not_terms.begin() + from, x.not_terms.end()), x.not_terms.end());
            x.not_at[q + 1] = x.not_terms.size();
        }
    }

    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    const ranked_args rk = ranked_args_of(wd, k, keys.data());
    const int st = or_queries_impl(qi, freqs_dict, should_terms, should_offsets, n_queries, counts, nullptr, nullptr, stream, ranked_extras(),
                                   &rk, &x);
    if (st != DINT_OK) return st;
    if (blocks_decoded) {
        *blocks_decoded = x.eager_blocks;
        for (const std::vector<uint32_t>& pass : x.step_claims)
            for (uint32_t n : pass) *blocks_decoded += n;
    }
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = x.h_matches[q];
        counts[q] = std::min<uint64_t>(x.h_matches[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
