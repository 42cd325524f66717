// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the ranked queries that report the
// most frequent values of a column over their matches and how many different values those have (DESIGN.md 4d-top-values).
// ---- top values and distinct counts of a value column over the matches of the ranked queries --------
// A top-values call is the filtered call (null filter: the ranged call on null ranges) with a top_values_args threaded through
// it: the same plan, the same launches, and in front of the selection an exact hash aggregation of the column over the slots
// of `cand` that the selection is about to read (dint_top_values_kernels.hpp) and a selection of its own over the tables, OR
// per pass behind the score kernel, AND behind the freqs pass's terms. The ranked outputs are therefore the filtered call's,
// bit for bit.

// What the top-values entries refuse of their own arguments, before any handle is dereferenced: only host pointers are looked at.
static bool top_values_host_args_ok(const dint_doc_values* values, uint32_t n_top, size_t n_queries, const uint64_t* value_counts,
                                    const uint64_t* distinct_counts, const uint32_t* top_n, const uint32_t* top_values,
                                    const uint32_t* top_counts) {
    if (!values || n_top > DINT_TOP_VALUES_MAX) return false;
    if (n_queries && (!value_counts || !distinct_counts || !top_n)) return false;
    return n_queries == 0 || n_top == 0 || (top_values && top_counts);
}

// What a top-values entry threads through its call beside rk: the ranged call on null ranges or the filtered call, as
// dint_ranked_or_filtered_queries chooses, and the aggregation's arguments.
struct top_values_call {
    restriction r;
    top_values_args tv;
    ranked_extras x;
    top_values_call(const dint_doc_filter* filter, const dint_doc_values* values, uint32_t n_top, size_t n_queries)
        : r(filter, nullptr, n_queries) {
        tv.values = values;
        tv.n_top = n_top;
        x.tv = &tv;
    }
    // Behind the call's last wait: the overflow word as a status — a table that ran full is a mistake of the library's, never
    // the caller's, and at a load of at most 1/2 it cannot happen — then the counts, a word each on the device, as the caller
    // takes them, and the selected keys count << 32 | ~value unpacked: query q's first min(n_top, distinct) keys hold a
    // value each, the outputs past them are 0.
    int outputs(size_t n_queries, uint64_t* value_counts, uint64_t* distinct_counts, uint32_t* top_n, uint32_t* top_values,
                uint32_t* top_counts) const {
        if (n_queries == 0) return DINT_OK;  // (nothing was planned: nothing to unpack)
        if (tv.h_words[2 * n_queries] != 0) return DINT_ERR_NOMEM;
        const uint32_t n_top = tv.n_top;
        for (size_t q = 0; q != n_queries; ++q) {
            value_counts[q] = tv.h_words[q];
            distinct_counts[q] = tv.h_words[n_queries + q];
            top_n[q] = std::min(n_top, tv.h_words[n_queries + q]);
            for (uint32_t i = 0; i != n_top; ++i) {
                const unsigned long long key = i < top_n[q] ? tv.h_keys[q * n_top + i] : 0ull;
                top_values[q * n_top + i] = key ? 0xFFFFFFFFu - uint32_t(key) : 0u;
                top_counts[q * n_top + i] = uint32_t(key >> 32);
            }
        }
        return DINT_OK;
    }
};

static int top_values_queries(bool conjunctive, dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                              const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                              const dint_doc_values* values, uint32_t n_top, size_t n_queries, uint64_t* counts, uint64_t* matches,
                              float* scores, uint32_t* docids, uint64_t* value_counts, uint64_t* distinct_counts, uint32_t* top_n,
                              uint32_t* top_values, uint32_t* top_counts, uint64_t* blocks_decoded, void* stream) {
    if (!top_values_host_args_ok(values, n_top, n_queries, value_counts, distinct_counts, top_n, top_values, top_counts) ||
        !ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || !value_stats_handles_ok(qi, filter, values))
        return DINT_ERR_ARG;
    top_values_call c(filter, values, n_top, n_queries);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(conjunctive, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries,
                                          counts, c.r, c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return c.outputs(n_queries, value_counts, distinct_counts, top_n, top_values, top_counts);
}

int dint_ranked_or_top_values_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                      const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                      const dint_doc_values* values, uint32_t n_top, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                      float* scores, uint32_t* docids, uint64_t* value_counts, uint64_t* distinct_counts, uint32_t* top_n,
                                      uint32_t* top_values, uint32_t* top_counts, uint64_t* blocks_decoded, void* stream) {
    return top_values_queries(false, qi, freqs_dict, wd, k, terms, query_offsets, filter, values, n_top, n_queries, counts, matches, scores,
                              docids, value_counts, distinct_counts, top_n, top_values, top_counts, blocks_decoded, stream);
}

int dint_ranked_and_top_values_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                       const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                       const dint_doc_values* values, uint32_t n_top, size_t n_queries, uint64_t* counts, uint64_t* matches,
                                       float* scores, uint32_t* docids, uint64_t* value_counts, uint64_t* distinct_counts, uint32_t* top_n,
                                       uint32_t* top_values, uint32_t* top_counts, uint64_t* blocks_decoded, void* stream) {
    return top_values_queries(true, qi, freqs_dict, wd, k, terms, query_offsets, filter, values, n_top, n_queries, counts, matches, scores,
                              docids, value_counts, distinct_counts, top_n, top_values, top_counts, blocks_decoded, stream);
}
