// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that return the
// hits behind a cursor (DESIGN.md 4d-paging).
// ---- search_after paging of the ranked queries ----------------------------------------------------
// A paged call is the filtered call (null filter: the ranged call on null ranges) or the collapsed call with a page_args
// threaded through it: the same plan, the same launches, and one more — page_after_kernel (dint_paging_kernels.hpp) over the
// slots of `cand` directly in front of ranked_topk, which kills every live slot that is not after its query's cursor and
// counts it. The selection then finds the best k of what is left. matches, collapsed, the facet rows and *blocks_decoded are
// therefore the un-paged call's, and every hit carries the score the un-paged call gives that document.

// The cursors as keys of the selection's order (collapse_key on the host), before anything is launched: null or +inf: from
// the start; a score <= 0 (-0.0f and -inf with it): nothing lies after it, every score is > 0. false: a NaN score.
static bool page_cursor_keys(const dint_rank_cursor* after, size_t n_queries, std::vector<unsigned long long>& keys) {
    keys.assign(n_queries, kPageFromStart);
    if (!after) return true;
    for (size_t q = 0; q != n_queries; ++q) {
        const float sc = after[q].score;
        if (std::isnan(sc)) return false;
        if (std::isinf(sc) && sc > 0.0f) continue;
        uint32_t bits = 0;
        std::memcpy(&bits, &sc, 4);
        keys[q] = sc <= 0.0f ? 0ull : (static_cast<unsigned long long>(bits) << 32) | (0xFFFFFFFFu - after[q].docid);
    }
    return true;
}

// the outputs of the plain entries from what their call brought back: h_matches[q] the matches, pg.h_skipped[q] those not
// after the cursor
static void paged_outputs(const page_args& pg, const std::vector<unsigned long long>& keys, size_t n_queries, uint32_t k,
                          const unsigned long long* h_matches, uint64_t* counts, uint64_t* matches, uint64_t* skipped, float* scores,
                          uint32_t* docids) {
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = h_matches[q];
        if (skipped) skipped[q] = pg.h_skipped[q];
        counts[q] = std::min<uint64_t>(h_matches[q] - pg.h_skipped[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
}

int dint_ranked_or_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                 const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                 const dint_rank_cursor* after, size_t n_queries, uint64_t* counts, uint64_t* matches, uint64_t* skipped,
                                 float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || (filter && filter->qi != qi)) return DINT_ERR_ARG;
    page_args pg;
    if (!page_cursor_keys(after, n_queries, pg.keys)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(filter, nullptr, n_queries);
    ranked_extras x;
    x.pg = &pg;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r, x,
                                          blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    paged_outputs(pg, keys, n_queries, k, h_matches.data(), counts, matches, skipped, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                  const dint_rank_cursor* after, size_t n_queries, uint64_t* counts, uint64_t* matches, uint64_t* skipped,
                                  float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || (filter && filter->qi != qi)) return DINT_ERR_ARG;
    page_args pg;
    if (!page_cursor_keys(after, n_queries, pg.keys)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(filter, nullptr, n_queries);
    ranked_extras x;
    x.pg = &pg;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r, x,
                                          blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    paged_outputs(pg, keys, n_queries, k, h_matches.data(), counts, matches, skipped, scores, docids);
    return DINT_OK;
}

// the outputs of the collapsed paged entries: as collapsed_outputs, with the kept documents not after the cursor taken off
static void collapsed_paged_outputs(const collapse_args& ca, const page_args& pg, const std::vector<unsigned long long>& keys, size_t n_queries,
                                    uint32_t k, const unsigned long long* h_matches, uint64_t* counts, uint64_t* matches, uint64_t* collapsed,
                                    uint64_t* skipped, float* scores, uint32_t* docids) {
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = h_matches[q];
        if (skipped) skipped[q] = pg.h_skipped[q];
        collapsed[q] = ca.h_collapsed[q];
        counts[q] = std::min<uint64_t>(ca.h_collapsed[q] - pg.h_skipped[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
}

int dint_ranked_or_collapsed_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                           const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                           const dint_doc_facets* facets, const dint_rank_cursor* after, size_t n_queries, uint64_t* counts,
                                           uint64_t* matches, uint64_t* collapsed, uint64_t* skipped, float* scores, uint32_t* docids,
                                           uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* facet_counts,
                                           uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !collapsed_args_ok(qi, filter, facets, n_queries, collapsed, hit_groups, hit_group_matches))
        return DINT_ERR_ARG;
    page_args pg;
    if (!page_cursor_keys(after, n_queries, pg.keys)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    collapsed_call c(filter, facets, n_queries, k, facet_counts, hit_groups, hit_group_matches);
    c.x.pg = &pg;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    collapsed_paged_outputs(c.ca, pg, keys, n_queries, k, h_matches.data(), counts, matches, collapsed, skipped, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_collapsed_paged_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                            const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                            const dint_doc_facets* facets, const dint_rank_cursor* after, size_t n_queries, uint64_t* counts,
                                            uint64_t* matches, uint64_t* collapsed, uint64_t* skipped, float* scores, uint32_t* docids,
                                            uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* facet_counts,
                                            uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !collapsed_args_ok(qi, filter, facets, n_queries, collapsed, hit_groups, hit_group_matches))
        return DINT_ERR_ARG;
    page_args pg;
    if (!page_cursor_keys(after, n_queries, pg.keys)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    collapsed_call c(filter, facets, n_queries, k, facet_counts, hit_groups, hit_group_matches);
    c.x.pg = &pg;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    collapsed_paged_outputs(c.ca, pg, keys, n_queries, k, h_matches.data(), counts, matches, collapsed, skipped, scores, docids);
    return DINT_OK;
}
