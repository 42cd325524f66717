// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": document-values handles, the ranked
// queries sorted by a column, and the value-range filter built on the device (DESIGN.md 4d-values).
// ---- document values: sorted ranked queries, value-range filters ------------------------------------
// A sorted call is the filtered call (null filter: the ranged call on null ranges) with a sort_args threaded through it: the
// same plan and the same scoring launches, so matches and *blocks_decoded are the filtered call's and every hit carries the
// score the filtered call gives that document. What differs lies around the selection (dint_doc_values_kernels.hpp):
// value_after_kernel cuts the slots at the cursor, ranked_topk sorts its runs by the key of the column's value, and
// sorted_hits_kernel recovers the selected hits' scores from the slots.

void dint_doc_values_destroy(dint_doc_values* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->d_values) (void)hipFree(v->d_values);
    delete v;
}

int dint_doc_values_create(int device, const uint32_t* values, uint64_t num_docs, dint_doc_values** out) {
    if (!out) return DINT_ERR_ARG;
    *out = nullptr;
    if (num_docs > 0xFFFFFFFFull || (num_docs && !values)) return DINT_ERR_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return DINT_ERR_NO_DEVICE;
    auto* v = new (std::nothrow) dint_doc_values();
    if (!v) return DINT_ERR_NOMEM;
    v->device = device;
    v->num_docs = num_docs;
    const bool ok = hip_ok(hipSetDevice(device), "hipSetDevice") &&
                    hip_ok(counted_malloc(&v->d_values, std::max<uint64_t>(1, num_docs) * 4), "counted_malloc(doc values)") &&
                    (num_docs == 0 || hip_ok(hipMemcpy(v->d_values, values, num_docs * 4, hipMemcpyHostToDevice), "hipMemcpy(doc values)"));
    if (!ok) {
        dint_doc_values_destroy(v);
        return DINT_ERR_HIP;
    }
    *out = v;
    return DINT_OK;
}

int dint_doc_values_info_get(const dint_doc_values* v, dint_doc_values_info* info) {
    if (!v || !info) return DINT_ERR_ARG;
    info->num_docs = v->num_docs;
    return DINT_OK;
}

int dint_doc_filter_create_from_values(dint_query_index* qi, const dint_doc_values* values, uint32_t lo, uint32_t hi, dint_doc_filter** out) {
    if (!qi || !out || !values || values->device != qi->device) return DINT_ERR_ARG;
    *out = nullptr;
    // the bitmap never exists on the host: a thread per document votes, a wave's ballot is a word of the handle's d_bits
    return doc_filter_build(qi, values->num_docs, [&](uint64_t* d_bits, uint64_t n_words) {
        hipLaunchKernelGGL(values_in_range_bits_kernel, dim3(uint32_t((n_words + 3) / 4)), dim3(256), 0, nullptr, values->view(), lo, hi, n_words,
                           d_bits);
        return hip_ok(hipGetLastError(), "values_in_range_bits_kernel");
    }, out);
}

// The sorted entries' own checks, before anything is dereferenced: the ranked entries' (scores are nullable here), the
// filtered entries', docids, the column and the order.
static bool sorted_args_ok(const dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                           const uint64_t* query_offsets, const dint_doc_filter* filter, const dint_doc_values* values, uint32_t order,
                           size_t n_queries, const uint64_t* counts, const uint32_t* docids) {
    static const float no_scores = 0.0f;  // (ranked_args_ok asks for scores)
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, &no_scores) || (filter && filter->qi != qi)) return false;
    if (n_queries && !docids) return false;
    return values && values->device == qi->device && order <= DINT_SORT_ASC;
}

// What a sorted entry threads through its call beside rk: the ranged call on null ranges or the filtered call, as
// dint_ranked_or_filtered_queries chooses, and the column, the order and the cursors as keys.
struct sorted_call {
    restriction r;
    sort_args sv;
    ranked_extras x;
    sorted_call(const dint_doc_filter* filter, const dint_doc_values* values, uint32_t order, uint32_t k, const dint_value_cursor* after,
                bool want_scores, size_t n_queries)
        : r(filter, nullptr, n_queries) {
        sv.values = values;
        sv.order = order;
        sv.k = k;
        sv.want_scores = want_scores;
        sv.keys.assign(n_queries, 0ull);
        sv.set.assign(n_queries, 0u);
        for (size_t q = 0; after && q != n_queries; ++q) {
            if (after[q].set == 0) continue;
            const uint32_t hi = order == DINT_SORT_ASC ? ~after[q].value : after[q].value;
            sv.keys[q] = (static_cast<unsigned long long>(hi) << 32) | (0xFFFFFFFFu - after[q].docid);
            sv.set[q] = 1;
            sv.any_set = true;
        }
        x.sv = &sv;
    }
};

// the outputs from what the call brought back: h_matches[q] the matches, sv.h_skipped[q] those not after the cursor, keys the
// selection's (K of every hit, descending), sv.h_hit_scores the hits' scores
static void sorted_outputs(const sort_args& sv, const std::vector<unsigned long long>& keys, size_t n_queries, uint32_t k,
                           const unsigned long long* h_matches, uint64_t* counts, uint64_t* matches, uint64_t* skipped, uint32_t* hit_values,
                           uint32_t* docids, float* scores) {
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = h_matches[q];
        if (skipped) skipped[q] = sv.h_skipped[q];
        counts[q] = std::min<uint64_t>(h_matches[q] - sv.h_skipped[q], k);
        for (uint32_t i = 0; i != k; ++i) {
            const bool hit = i < counts[q];
            const unsigned long long key = keys[q * k + i];
            const uint32_t hi = uint32_t(key >> 32);
            docids[q * k + i] = hit ? 0xFFFFFFFFu - uint32_t(key) : 0xFFFFFFFFu;
            if (hit_values) hit_values[q * k + i] = hit ? (sv.order == DINT_SORT_ASC ? ~hi : hi) : 0u;
            if (scores) scores[q * k + i] = hit ? sv.h_hit_scores[q * k + i] : 0.0f;
        }
    }
}

int dint_ranked_or_sorted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                  const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                  const dint_doc_values* values, uint32_t order, const dint_value_cursor* after, size_t n_queries,
                                  uint64_t* counts, uint64_t* matches, uint64_t* skipped, uint32_t* hit_values, uint32_t* docids, float* scores,
                                  uint64_t* blocks_decoded, void* stream) {
    if (!sorted_args_ok(qi, freqs_dict, wd, k, query_offsets, filter, values, order, n_queries, counts, docids)) return DINT_ERR_ARG;
    sorted_call c(filter, values, order, k, after, scores != nullptr, n_queries);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    sorted_outputs(c.sv, keys, n_queries, k, h_matches.data(), counts, matches, skipped, hit_values, docids, scores);
    return DINT_OK;
}

int dint_ranked_and_sorted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                   const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                   const dint_doc_values* values, uint32_t order, const dint_value_cursor* after, size_t n_queries,
                                   uint64_t* counts, uint64_t* matches, uint64_t* skipped, uint32_t* hit_values, uint32_t* docids, float* scores,
                                   uint64_t* blocks_decoded, void* stream) {
    if (!sorted_args_ok(qi, freqs_dict, wd, k, query_offsets, filter, values, order, n_queries, counts, docids)) return DINT_ERR_ARG;
    sorted_call c(filter, values, order, k, after, scores != nullptr, n_queries);
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, c.r,
                                          c.x, blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    sorted_outputs(c.sv, keys, n_queries, k, h_matches.data(), counts, matches, skipped, hit_values, docids, scores);
    return DINT_OK;
}
