// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": ranked disjunctive queries
// (ranked_or_query, queries.hpp:387-457).
// ---- ranked disjunctive queries -----------------------------------------------------------------
// A ranked OR call is an or_query<true> call (or_queries_impl) whose probe launch scores instead of counting: per pass,
// ranked_or_score_kernel (dint_ranked_or_query_kernels.hpp) gives every document of a query's union its whole score at
// its first occurrence, and ranked_topk selects the k best of every query of the pass. The workspaces and the lock are
// the AND and OR calls' own; the AND claim tables are not touched.

int dint_ranked_or_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                           const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts, float* scores,
                           uint32_t* docids, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    const ranked_args rk = ranked_args_of(wd, k, keys.data());
    // (or_queries_impl checks the offsets and the terms before anything is launched)
    const int st = or_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream, ranked_extras(), &rk);
    if (st != DINT_OK) return st;
    counts_from_keys(keys, n_queries, k, counts);
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
