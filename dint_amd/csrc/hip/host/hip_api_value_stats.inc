// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that reduce a
// column's values over their matches (DESIGN.md 4d-stats).
// ---- value statistics and range histograms of the ranked queries ------------------------------------
// A value-stats call is the filtered call (null filter: the ranged call on null ranges) with a value_stats_args threaded
// through it: the same plan, the same launches, and one more in front of the selection — value_stats_kernel
// (dint_value_stats_kernels.hpp) over the slots of `cand` that the selection is about to read, OR per pass behind the score
// kernel, AND behind the freqs pass's terms — and, where the caller asks for the hits' values, hit_values_kernel behind it.
// The ranked outputs are therefore the filtered call's, bit for bit.

// What the value-stats entries refuse of their own arguments, before any handle is dereferenced: only host arrays are read.
static bool value_stats_host_args_ok(const dint_doc_values* values, const uint32_t* edges, uint32_t n_edges, size_t n_queries,
                                     const dint_value_stats* stats, const uint32_t* bucket_counts) {
    if (!values || !stats || n_edges > DINT_VALUE_STATS_MAX_EDGES) return false;
    if (n_edges && (!edges || !bucket_counts)) return false;
    for (uint32_t i = 1; i < n_edges; ++i)
        if (edges[i - 1] >= edges[i]) return false;
    return uint64_t(n_queries) <= (uint64_t(1) << 28) / (uint64_t(n_edges) + 1);  // n_queries * (n_edges + 1) <= 2^28
}

// ... and of the handles, behind the ranked entries' own checks: a filter of another index, a column on another device
static bool value_stats_handles_ok(const dint_query_index* qi, const dint_doc_filter* filter, const dint_doc_values* values) {
    return (!filter || filter->qi == qi) && values->device == qi->docs->device;
}

// What a value-stats entry threads through its call beside rk: the ranged call on null ranges or the filtered call, as
// dint_ranked_or_filtered_queries chooses, and the column, the edges and the caller's outputs.
struct value_stats_call {
    restriction r;
    value_stats_args vs;
    ranked_extras x;
    value_stats_call(const dint_doc_filter* filter, const dint_doc_values* values, const uint32_t* edges, uint32_t n_edges, uint32_t k,
                     size_t n_queries, dint_value_stats* stats, uint32_t* bucket_counts, uint32_t* hit_values)
        : r(filter, nullptr, n_queries) {
        vs.values = values;
        vs.edges = edges;
        vs.n_edges = n_edges;
        vs.k = k;
        vs.h_stats = stats;
        vs.h_rows = bucket_counts;
        vs.h_hit_values = hit_values;
        x.vs = &vs;
    }
};

int dint_ranked_or_value_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_values* values, const uint32_t* edges, uint32_t n_edges, size_t n_queries,
                                       uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* stats,
                                       uint32_t* bucket_counts, uint32_t* hit_values, uint64_t* blocks_decoded, void* stream) {
    if (!value_stats_host_args_ok(values, edges, n_edges, n_queries, stats, bucket_counts) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || !value_stats_handles_ok(qi, filter, values))
        return DINT_ERR_ARG;
    value_stats_call c(filter, values, edges, n_edges, k, n_queries, stats, bucket_counts, hit_values);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_value_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                        const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                        const dint_doc_values* values, const uint32_t* edges, uint32_t n_edges, size_t n_queries,
                                        uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* stats,
                                        uint32_t* bucket_counts, uint32_t* hit_values, uint64_t* blocks_decoded, void* stream) {
    if (!value_stats_host_args_ok(values, edges, n_edges, n_queries, stats, bucket_counts) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || !value_stats_handles_ok(qi, filter, values))
        return DINT_ERR_ARG;
    value_stats_call c(filter, values, edges, n_edges, k, n_queries, stats, bucket_counts, hit_values);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}
