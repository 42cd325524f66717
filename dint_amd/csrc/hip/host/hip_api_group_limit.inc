// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that return up
// to per_group documents of every document group (DESIGN.md 4d-group-limit).
// ---- group-limited ranked queries -----------------------------------------------------------------
// A group-limited call is the faceted call with a group_limit_args threaded through it beside its facet_args, and a page_args
// where the caller gives a cursor: the same plan, the same launches, and per_group + 2 more (dint_group_limit_kernels.hpp) —
// the rounds of group_limit_round_kernel and group_limit_keep_kernel between facet_count_kernel and page_after_kernel /
// ranked_topk, over the slots of `cand` that the selection is about to read, and group_limit_hits_kernel behind it, over the
// keys it selected. The facet rows are always counted on the device (group_limit_hits_kernel reads them) and copied to the
// host only where the caller gives facet_counts. matches and *blocks_decoded are therefore the faceted call's, the cursor
// applies to the kept documents as the collapsed paged entries apply it, and every kept hit carries the score the unfiltered
// call gives that document.

// What the group-limited entries refuse without reading a handle — these checks come first: a null handle or required
// output, a k or per_group out of range, a NaN cursor, and a batch that is too large whatever the map (a map has at least
// one group, so n_queries * per_group > 2^27 is past the table's cap).
static bool group_limit_plain_args_ok(const void* qi, const void* freqs_dict, const void* wd, uint32_t k, const uint64_t* query_offsets,
                                      const void* facets, uint32_t per_group, const dint_rank_cursor* after, size_t n_queries,
                                      const uint64_t* counts, const uint64_t* kept, const float* scores, const uint32_t* hit_groups,
                                      const uint32_t* hit_group_matches, const uint32_t* hit_group_ranks) {
    if (!qi || !freqs_dict || !wd || !facets || k == 0 || k > kRankedMaxK) return false;
    if (n_queries && (!query_offsets || !counts || !scores)) return false;
    if (!kept || !hit_groups || !hit_group_matches || !hit_group_ranks) return false;
    if (per_group == 0 || per_group > DINT_GROUP_LIMIT_MAX || uint64_t(n_queries) > (uint64_t(1) << 27) / per_group) return false;
    for (size_t q = 0; after && q != n_queries; ++q)
        if (std::isnan(after[q].score)) return false;
    return true;
}
// ... and what they refuse of their handles, besides the collapsed entries' own: before anything is written or launched
static bool group_limit_args_ok(const dint_query_index* qi, const dint_doc_filter* filter, const dint_doc_facets* facets, uint32_t per_group,
                                size_t n_queries, const uint64_t* kept, const uint32_t* hit_groups, const uint32_t* hit_group_matches) {
    if (!collapsed_args_ok(qi, filter, facets, n_queries, kept, hit_groups, hit_group_matches)) return false;
    // (n_queries * n_groups <= 2^27 and per_group <= 16: the product cannot wrap)
    return uint64_t(n_queries) * facets->n_groups * per_group <= (uint64_t(1) << 27);
}

// the outputs of either entry from what its call brought back: h_matches[q] the matches, gl.h_kept[q] the kept documents,
// pg.h_skipped[q] the kept documents not after the cursor
static void group_limit_outputs(const group_limit_args& gl, const page_args& pg, const std::vector<unsigned long long>& keys, size_t n_queries,
                                uint32_t k, const unsigned long long* h_matches, uint64_t* counts, uint64_t* matches, uint64_t* kept,
                                uint64_t* skipped, float* scores, uint32_t* docids) {
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = h_matches[q];
        if (skipped) skipped[q] = pg.h_skipped[q];
        kept[q] = gl.h_kept[q];
        counts[q] = std::min<uint64_t>(gl.h_kept[q] - pg.h_skipped[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
}

// What either entry threads through its call beside rk: the ranged call on null ranges or the filtered call (as the faceted
// entries have it), the facet rows — kept on the device where facet_counts is null —, the limit itself and the cursors.
struct group_limit_call {
    restriction r;
    facet_args fa;
    group_limit_args gl;
    page_args pg;
    ranked_extras x;
    group_limit_call(const dint_doc_filter* filter, const dint_doc_facets* facets, size_t n_queries, uint32_t k, uint32_t per_group,
                     uint32_t* facet_counts, uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* hit_group_ranks)
        : r(filter, nullptr, n_queries) {
        fa.facets = facets;
        fa.h_rows = facet_counts;
        gl.per_group = per_group;
        gl.k = k;
        gl.h_hit_groups = hit_groups;
        gl.h_hit_group_matches = hit_group_matches;
        gl.h_hit_group_ranks = hit_group_ranks;
        x.fa = &fa;
        x.gl = &gl;
    }
    // the cursors as keys; false: a NaN score. A call whose every query reads from the start threads no page_args at all:
    // page_after_kernel runs only where a cursor is given.
    bool cursors(const dint_rank_cursor* after, size_t n_queries) {
        if (!page_cursor_keys(after, n_queries, pg.keys)) return false;
        const bool paged = std::any_of(pg.keys.begin(), pg.keys.end(), [](unsigned long long key) { return key != kPageFromStart; });
        x.pg = paged ? &pg : nullptr;
        pg.h_skipped.assign(n_queries, 0ull);
        return true;
    }
};

int dint_ranked_or_group_limit_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_facets* facets, uint32_t per_group, const dint_rank_cursor* after, size_t n_queries,
                                       uint64_t* counts, uint64_t* matches, uint64_t* kept, uint64_t* skipped, float* scores,
                                       uint32_t* docids, uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* hit_group_ranks,
                                       uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!group_limit_plain_args_ok(qi, freqs_dict, wd, k, query_offsets, facets, per_group, after, n_queries, counts, kept, scores, hit_groups,
                                   hit_group_matches, hit_group_ranks) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !group_limit_args_ok(qi, filter, facets, per_group, n_queries, kept, hit_groups, hit_group_matches))
        return DINT_ERR_ARG;
    group_limit_call c(filter, facets, n_queries, k, per_group, facet_counts, hit_groups, hit_group_matches, hit_group_ranks);
    if (!c.cursors(after, n_queries)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    group_limit_outputs(c.gl, c.pg, keys, n_queries, k, h_matches.data(), counts, matches, kept, skipped, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_group_limit_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                        const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                        const dint_doc_facets* facets, uint32_t per_group, const dint_rank_cursor* after, size_t n_queries,
                                        uint64_t* counts, uint64_t* matches, uint64_t* kept, uint64_t* skipped, float* scores,
                                        uint32_t* docids, uint32_t* hit_groups, uint32_t* hit_group_matches, uint32_t* hit_group_ranks,
                                        uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!group_limit_plain_args_ok(qi, freqs_dict, wd, k, query_offsets, facets, per_group, after, n_queries, counts, kept, scores, hit_groups,
                                   hit_group_matches, hit_group_ranks) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !group_limit_args_ok(qi, filter, facets, per_group, n_queries, kept, hit_groups, hit_group_matches))
        return DINT_ERR_ARG;
    group_limit_call c(filter, facets, n_queries, k, per_group, facet_counts, hit_groups, hit_group_matches, hit_group_ranks);
    if (!c.cursors(after, n_queries)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    group_limit_outputs(c.gl, c.pg, keys, n_queries, k, h_matches.data(), counts, matches, kept, skipped, scores, docids);
    return DINT_OK;
}
