// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that return the
// best document of every document group (DESIGN.md 4d-collapse).
// ---- collapsed ranked queries ---------------------------------------------------------------------
// A collapsed call is the faceted call with a collapse_args threaded through it beside its facet_args: the same plan, the
// same launches, and three more (dint_collapse_kernels.hpp) — collapse_best_kernel and collapse_keep_kernel between
// facet_count_kernel and ranked_topk, over the slots of `cand` that the selection is about to read, and collapse_hits_kernel
// behind it, over the keys it selected. The facet rows are always counted on the device (collapse_hits_kernel reads them)
// and copied to the host only where the caller gives facet_counts. matches and *blocks_decoded are therefore the faceted
// call's, and every kept hit carries the score the unfiltered call gives that document.

// what the collapsed entries refuse besides the filtered entries' own: before anything is written or launched
static bool collapsed_args_ok(const dint_query_index* qi, const dint_doc_filter* filter, const dint_doc_facets* facets, size_t n_queries,
                              const uint64_t* collapsed, const uint32_t* hit_groups, const uint32_t* hit_group_matches) {
    if (!facets || !collapsed || !hit_groups || !hit_group_matches || (filter && filter->qi != qi)) return false;
    return facets->device == qi->docs->device && uint64_t(n_queries) * facets->n_groups <= (uint64_t(1) << 27);
}

// the outputs of either entry from what its call brought back: h_matches[q] the matches, ca.h_collapsed[q] the kept documents
static void collapsed_outputs(const collapse_args& ca, const std::vector<unsigned long long>& keys, size_t n_queries, uint32_t k,
                              const unsigned long long* h_matches, uint64_t* counts, uint64_t* matches, uint64_t* collapsed, float* scores,
                              uint32_t* docids) {
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = h_matches[q];
        collapsed[q] = ca.h_collapsed[q];
        counts[q] = std::min<uint64_t>(ca.h_collapsed[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
}

// What either entry threads through its call beside rk: the ranged call on null ranges or the filtered call (as the faceted
// entries have it), the facet rows — kept on the device where facet_counts is null — and the collapse itself.
struct collapsed_call {
    restriction r;
    facet_args fa;
    collapse_args ca;
    ranked_extras x;
    collapsed_call(const dint_doc_filter* filter, const dint_doc_facets* facets, size_t n_queries, uint32_t k, uint32_t* facet_counts,
                   uint32_t* hit_groups, uint32_t* hit_group_matches)
        : r(filter, nullptr, n_queries) {
        fa.facets = facets;
        fa.h_rows = facet_counts;
        ca.k = k;
        ca.h_hit_groups = hit_groups;
        ca.h_hit_group_matches = hit_group_matches;
        x.fa = &fa;
        x.ca = &ca;
    }
};

int dint_ranked_or_collapsed_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                     const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                     const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                     uint64_t* collapsed, float* scores, uint32_t* docids, uint32_t* hit_groups,
                                     uint32_t* hit_group_matches, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !collapsed_args_ok(qi, filter, facets, n_queries, collapsed, hit_groups, hit_group_matches))
        return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    collapsed_call c(filter, facets, n_queries, k, facet_counts, hit_groups, hit_group_matches);
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    collapsed_outputs(c.ca, keys, n_queries, k, h_matches.data(), counts, matches, collapsed, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_collapsed_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                      const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                      const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                      uint64_t* collapsed, float* scores, uint32_t* docids, uint32_t* hit_groups,
                                      uint32_t* hit_group_matches, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !collapsed_args_ok(qi, filter, facets, n_queries, collapsed, hit_groups, hit_group_matches))
        return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    collapsed_call c(filter, facets, n_queries, k, facet_counts, hit_groups, hit_group_matches);
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    collapsed_outputs(c.ca, keys, n_queries, k, h_matches.data(), counts, matches, collapsed, scores, docids);
    return DINT_OK;
}
