// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that select
// exact percentiles of a column's values over their matches (DESIGN.md 4d-percentiles).
// ---- exact percentiles of a value column over the matches of the ranked queries ---------------------
// A percentile call is the filtered call (null filter: the ranged call on null ranges) with a percentile_args threaded
// through it: the same plan, the same launches, and in front of the selection the four rounds of a radix select
// (dint_percentile_kernels.hpp) over the slots of `cand` that the selection is about to read, OR per pass behind the score
// kernel, AND behind the freqs pass's terms. Where the caller asks for the statistics too, a value_stats_args with no edges
// and no hit values travels beside it: exactly the value-stats call's launch. The ranked outputs are therefore the filtered
// call's, bit for bit.

// What the percentile entries refuse of their own arguments, before any handle is dereferenced: only host arrays are read.
static bool percentile_host_args_ok(const dint_doc_values* values, const uint32_t* per_million, uint32_t n_percentiles, size_t n_queries,
                                    const uint64_t* value_counts, const uint32_t* percentile_values) {
    if (!values || !per_million || !value_counts || !percentile_values) return false;
    if (n_percentiles == 0 || n_percentiles > DINT_PERCENTILES_MAX) return false;
    for (uint32_t j = 0; j != n_percentiles; ++j)
        if (per_million[j] > 1000000u) return false;
    return uint64_t(n_queries) <= DINT_PERCENTILES_MAX_RECORDS / n_percentiles;  // n_queries * n_percentiles <= the cap
}

// What a percentile entry threads through its call beside rk: the ranged call on null ranges or the filtered call, as
// dint_ranked_or_filtered_queries chooses, the select's arguments and, where stats is given, the value-stats call's.
struct percentile_call {
    restriction r;
    value_stats_args vs;
    percentile_args pa;
    ranked_extras x;
    percentile_call(const dint_doc_filter* filter, const dint_doc_values* values, const uint32_t* per_million, uint32_t n_percentiles,
                    uint32_t k, size_t n_queries, uint64_t* value_counts, uint32_t* percentile_values, dint_value_stats* stats)
        : r(filter, nullptr, n_queries) {
        pa.values = values;
        pa.per_million = per_million;
        pa.n_p = n_percentiles;
        pa.h_value_counts = value_counts;
        pa.h_values = percentile_values;
        vs.values = values;
        vs.k = k;
        vs.h_stats = stats;
        x.vs = stats ? &vs : nullptr;  // (null: nothing of the value-stats machinery runs)
        x.pa = &pa;
    }
    // behind the call's last wait: the counts, a word each on the device, as the caller takes them
    void widen_counts(size_t n_queries) {
        for (size_t q = 0; q != n_queries; ++q) pa.h_value_counts[q] = pa.h_n[q];
    }
};

int dint_ranked_or_percentile_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                      const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                      const dint_doc_values* values, const uint32_t* per_million, uint32_t n_percentiles, size_t n_queries,
                                      uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* value_counts,
                                      uint32_t* percentile_values, dint_value_stats* stats, uint64_t* blocks_decoded, void* stream) {
    if (!percentile_host_args_ok(values, per_million, n_percentiles, n_queries, value_counts, percentile_values) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || !value_stats_handles_ok(qi, filter, values))
        return DINT_ERR_ARG;
    percentile_call c(filter, values, per_million, n_percentiles, k, n_queries, value_counts, percentile_values, stats);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    c.widen_counts(n_queries);
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_percentile_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_values* values, const uint32_t* per_million, uint32_t n_percentiles, size_t n_queries,
                                       uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* value_counts,
                                       uint32_t* percentile_values, dint_value_stats* stats, uint64_t* blocks_decoded, void* stream) {
    if (!percentile_host_args_ok(values, per_million, n_percentiles, n_queries, value_counts, percentile_values) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || !value_stats_handles_ok(qi, filter, values))
        return DINT_ERR_ARG;
    percentile_call c(filter, values, per_million, n_percentiles, k, n_queries, value_counts, percentile_values, stats);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    c.widen_counts(n_queries);
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}
