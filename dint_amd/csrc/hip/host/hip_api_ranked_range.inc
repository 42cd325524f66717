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

// How a call is restricted, as the ranged, the filtered and every later family's entries have it: by the filter where one is
// given, else by the ranges (null: every query unrestricted — the unfiltered call with the matches counted). One of
// ranged() / filtered() goes into the call; blocks() and h_matches() are what that one brought back.
struct restriction {
    std::vector<dint_doc_range> all;
    range_args rg;
    filter_args fl;
    restriction(const dint_doc_filter* filter, const dint_doc_range* ranges, size_t n_queries) {
        if (filter)
            fl.filter = filter;
        else
            rg.ranges = ranges_or_all(ranges, n_queries, all);
    }
    restriction(const restriction&) = delete;  // (rg.ranges may point into all)
    range_args* ranged() { return fl.filter ? nullptr : &rg; }
    filter_args* filtered() { return fl.filter ? &fl : nullptr; }
    uint64_t blocks() const { return fl.filter ? fl.blocks : rg.blocks; }
    std::vector<unsigned long long>& h_matches() { return fl.filter ? fl.h_matches : rg.h_matches; }
};

// One restricted ranked call with its extras, as the union of the queries' lists or (conjunctive) their intersection. The
// impl checks the offsets and the terms before anything is written or launched. *blocks_decoded (if given) <- the pages the
// call planned; h_matches <- per query the matches: OR counts them into the restriction's counters, AND's counts are the
// survivors of the rounds, which run behind the restriction's kill and in front of every extra's.
static int ranked_restricted_call(bool conjunctive, dint_query_index* qi, const dint_dict* freqs_dict, const ranked_args& rk,
                                  const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts, restriction& r,
                                  const ranked_extras& x, uint64_t* blocks_decoded, std::vector<unsigned long long>& h_matches, void* stream) {
    if (conjunctive) {
        std::vector<uint64_t> freq_sums(n_queries, 0);
        const int st = and_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums.data(), nullptr, stream, x, false, &rk,
                                        nullptr, r.ranged(), r.filtered());
        if (st != DINT_OK) return st;
        h_matches.assign(counts, counts + n_queries);
    } else {
        const int st = or_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream, x, &rk, nullptr,
                                       r.ranged(), r.filtered());
        if (st != DINT_OK) return st;
        h_matches.swap(r.h_matches());
    }
    if (blocks_decoded) *blocks_decoded = r.blocks();
    return DINT_OK;
}

// the outputs of an entry whose extras leave the selection alone: every match is selected from
static void restricted_outputs(const std::vector<unsigned long long>& keys, size_t n_queries, uint32_t k,
                               const std::vector<unsigned long long>& h_matches, uint64_t* counts, uint64_t* matches, float* scores,
                               uint32_t* docids) {
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = h_matches[q];
        counts[q] = std::min<uint64_t>(h_matches[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
}

int dint_ranked_or_range_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                 const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_range* ranges, size_t n_queries,
                                 uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded,
                                 void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(nullptr, ranges, n_queries);
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r,
                                          ranked_extras(), blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_range_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_range* ranges, size_t n_queries,
                                  uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded,
                                  void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(nullptr, ranges, n_queries);
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r,
                                          ranked_extras(), blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}
