// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": docID-range ranked queries
// (ranked_or_query / ranked_and_query, queries.hpp:309-457, over the documents of a half-open docID interval per query).
// ---- docID-range ranked queries -------------------------------------------------------------------
// A ranged call is the unranged call (or_queries_impl / and_queries_impl with rk) with a range_args threaded through it
// (DESIGN.md 4d-range): the host plans only the blocks that can hold a docID of the query's range (blocks_in_range, over
// the handle's host copy of the block maxima), and a kernel of dint_ranked_range_kernels.hpp retires what the boundary
// blocks hold outside it — OR: ranked_or_range_score_kernel in place of ranked_or_score_kernel; AND: range_kill_kernel
// between the candidates' decode and the first round's search. The query weights come from the whole lists' lengths, so a
// match scores what the unranged call gives it. The selection, the workspaces and the lock are the unranged calls' own.

// the call's ranges: the caller's, or (null) every query unrestricted, held in `all`
static const dint_doc_range* ranges_or_all(const dint_doc_range* ranges, size_t n_queries, std::vector<dint_doc_range>& all) {
    if (ranges) return ranges;
    all.assign(n_queries, dint_doc_range{0u, 0xFFFFFFFFu});
    return all.data();
}

int dint_ranked_or_range_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                 const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_range* ranges, size_t n_queries,
                                 uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded,
                                 void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    const ranked_args rk = ranked_args_of(wd, k, keys.data());
    std::vector<dint_doc_range> all;
    range_args rg;
    rg.ranges = ranges_or_all(ranges, n_queries, all);
    // (or_queries_impl checks the offsets and the terms before anything is written or launched)
    const int st = or_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream, &rk, nullptr, &rg);
    if (st != DINT_OK) return st;
    if (blocks_decoded) *blocks_decoded = rg.blocks;
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = rg.h_matches[q];
        counts[q] = std::min<uint64_t>(rg.h_matches[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_range_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_range* ranges, size_t n_queries,
                                  uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded,
                                  void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    std::vector<uint64_t> freq_sums(n_queries, 0);
    const ranked_args rk = ranked_args_of(wd, k, keys.data());
    std::vector<dint_doc_range> all;
    range_args rg;
    rg.ranges = ranges_or_all(ranges, n_queries, all);
    // (and_queries_impl checks the offsets and the terms before anything is written or launched; its counts are the
    // survivors of the rounds, which run behind the kill: the matches in range)
    const int st = and_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums.data(), nullptr, stream, false, &rk,
                                    nullptr, &rg);
    if (st != DINT_OK) return st;
    if (blocks_decoded) *blocks_decoded = rg.blocks;
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = counts[q];
        counts[q] = std::min<uint64_t>(counts[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
