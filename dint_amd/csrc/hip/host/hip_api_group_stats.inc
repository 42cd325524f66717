// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that reduce a
// column's values over their matches per document group (DESIGN.md 4d-group-stats).
// ---- per-group value statistics of the ranked queries ---------------------------------------------
// A group-stats call is the filtered call (null filter: the ranged call on null ranges) with a group_stats_args threaded
// through it: the same plan, the same launches, and one more in front of the selection — group_stats_kernel
// (dint_group_stats_kernels.hpp) over the slots of `cand` that the selection is about to read, OR per pass behind the score
// kernel, AND behind the freqs pass's terms. Where the caller asks for the facet rows too, the faceted call's facet_args
// travels beside it and facet_count_kernel runs as it does there. The ranked outputs are therefore the filtered call's, and
// the rows the faceted call's, bit for bit.

// What the group-stats entries refuse of their own arguments, before any handle is dereferenced
static bool group_stats_host_args_ok(const dint_doc_facets* facets, const dint_doc_values* values, const dint_value_stats* group_stats) {
    return facets && values && group_stats;
}

// ... and of the handles, behind the ranked entries' own checks: a filter of another index, a map or a column on another
// device, more records than a call takes. Only the handles are read: no array of the caller's.
static bool group_stats_handles_ok(const dint_query_index* qi, const dint_doc_filter* filter, const dint_doc_facets* facets,
                                   const dint_doc_values* values, size_t n_queries) {
    if (filter && filter->qi != qi) return false;
    if (facets->device != qi->docs->device || values->device != qi->docs->device) return false;
    return uint64_t(n_queries) <= DINT_GROUP_STATS_MAX_RECORDS / facets->n_groups;  // n_queries * n_groups <= 2^24 (n_groups >= 1)
}

// What a group-stats entry threads through its call beside rk: the ranged call on null ranges or the filtered call, as
// dint_ranked_or_filtered_queries chooses, the map, the column and the caller's records, and the faceted call's rows where
// the caller takes them.
struct group_stats_call {
    restriction r;
    facet_args fa;
    group_stats_args gs;
    ranked_extras x;
    group_stats_call(const dint_doc_filter* filter, const dint_doc_facets* facets, const dint_doc_values* values, size_t n_queries,
                     dint_value_stats* group_stats, uint32_t* facet_counts)
        : r(filter, nullptr, n_queries) {
        fa.facets = facets;
        fa.h_rows = facet_counts;
        gs.facets = facets;
        gs.values = values;
        gs.h_recs = group_stats;
        x.fa = facet_counts ? &fa : nullptr;
        x.gs = &gs;
    }
};

int dint_ranked_or_group_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_facets* facets, const dint_doc_values* values, size_t n_queries, uint64_t* counts,
                                       uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* group_stats,
                                       uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!group_stats_host_args_ok(facets, values, group_stats) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !group_stats_handles_ok(qi, filter, facets, values, n_queries))
        return DINT_ERR_ARG;
    group_stats_call c(filter, facets, values, n_queries, group_stats, facet_counts);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_group_stats_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                        const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                        const dint_doc_facets* facets, const dint_doc_values* values, size_t n_queries, uint64_t* counts,
                                        uint64_t* matches, float* scores, uint32_t* docids, dint_value_stats* group_stats,
                                        uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!group_stats_host_args_ok(facets, values, group_stats) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !group_stats_handles_ok(qi, filter, facets, values, n_queries))
        return DINT_ERR_ARG;
    group_stats_call c(filter, facets, values, n_queries, group_stats, facet_counts);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}
