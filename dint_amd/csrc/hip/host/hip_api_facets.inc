// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": facets handles and the ranked
// queries that count their matches per document group (DESIGN.md 4d-facets).
// ---- faceted ranked queries -----------------------------------------------------------------------
// A faceted call is the filtered call (null filter: the ranged call on null ranges) with a facet_args threaded through it:
// the same plan, the same launches, and one more — facet_count_kernel (dint_facet_kernels.hpp) over the slots of `cand` that
// the selection is about to read, OR per pass behind the score kernel, AND behind the freqs pass's terms. It adds to the
// call's rows in the index's facet_rows workspace, which come back with the matches. The ranked outputs are therefore the
// filtered call's, bit for bit.

void dint_doc_facets_destroy(dint_doc_facets* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->d_group_of) (void)hipFree(f->d_group_of);
    delete f;
}

int dint_doc_facets_create(int device, const uint32_t* group_of, uint64_t num_docs, uint32_t n_groups, dint_doc_facets** out) {
    if (!out) return DINT_ERR_ARG;
    *out = nullptr;
    if (n_groups == 0 || n_groups > DINT_FACETS_MAX_GROUPS || num_docs > 0xFFFFFFFFull || (num_docs && !group_of)) return DINT_ERR_ARG;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return DINT_ERR_NO_DEVICE;
    auto* f = new (std::nothrow) dint_doc_facets();
    if (!f) return DINT_ERR_NOMEM;
    f->device = device;
    f->num_docs = num_docs;
    f->n_groups = n_groups;
    try {
        f->sizes.assign(size_t(n_groups) + 1, 0u);  // (the kernel's invalid flag behind the sizes, until it is read)
    } catch (const std::bad_alloc&) {
        delete f;
        return DINT_ERR_NOMEM;
    }
    // the creation's own memory: the sizes and, behind them, the invalid flag
    uint32_t* d_sizes = nullptr;
    bool ok = hip_ok(hipSetDevice(device), "hipSetDevice") &&
              hip_ok(counted_malloc(&f->d_group_of, std::max<uint64_t>(1, num_docs) * 4), "counted_malloc(group_of)") &&
              hip_ok(counted_malloc(&d_sizes, (size_t(n_groups) + 1) * 4), "counted_malloc(group sizes)") &&
              hip_ok(hipMemset(d_sizes, 0, (size_t(n_groups) + 1) * 4), "hipMemset(group sizes)") &&
              (num_docs == 0 || hip_ok(hipMemcpy(f->d_group_of, group_of, num_docs * 4, hipMemcpyHostToDevice), "hipMemcpy(group_of)"));
    if (ok && num_docs) {
        hipLaunchKernelGGL(facet_group_sizes_kernel, dim3(uint32_t((num_docs + 255) / 256)), dim3(256), 0, nullptr, f->d_group_of, num_docs,
                           n_groups, d_sizes, d_sizes + n_groups);
        ok = hip_ok(hipGetLastError(), "facet_group_sizes_kernel");
    }
    ok = ok && hip_ok(hipMemcpy(f->sizes.data(), d_sizes, (size_t(n_groups) + 1) * 4, hipMemcpyDeviceToHost), "hipMemcpy(group sizes)");
    if (d_sizes) (void)hipFree(d_sizes);
    if (!ok) {
        dint_doc_facets_destroy(f);
        return DINT_ERR_HIP;
    }
    const bool invalid = f->sizes[n_groups] != 0;
    f->sizes.pop_back();
    if (invalid) {  // (an entry that is neither a group nor DINT_FACET_NONE)
        dint_doc_facets_destroy(f);
        return DINT_ERR_ARG;
    }
    for (uint32_t n : f->sizes) f->n_grouped += n;
    *out = f;
    return DINT_OK;
}

int dint_doc_facets_info_get(const dint_doc_facets* f, dint_doc_facets_info* info) {
    if (!f || !info) return DINT_ERR_ARG;
    info->num_docs = f->num_docs;
    info->n_groups = f->n_groups;
    info->n_grouped = f->n_grouped;
    return DINT_OK;
}

int dint_doc_facets_group_sizes(const dint_doc_facets* f, uint32_t* sizes) {
    if (!f || !sizes) return DINT_ERR_ARG;
    std::copy(f->sizes.begin(), f->sizes.end(), sizes);
    return DINT_OK;
}

// what the faceted entries refuse besides the filtered entries' own: before anything is written or launched
static bool faceted_args_ok(const dint_query_index* qi, const dint_doc_filter* filter, const dint_doc_facets* facets, size_t n_queries,
                            const uint32_t* facet_counts) {
    if (!facets || !facet_counts || (filter && filter->qi != qi)) return false;
    return facets->device == qi->docs->device && uint64_t(n_queries) * facets->n_groups <= (uint64_t(1) << 28);
}

int dint_ranked_or_faceted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                   const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                   const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores,
                                   uint32_t* docids, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !faceted_args_ok(qi, filter, facets, n_queries, facet_counts))
        return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(filter, nullptr, n_queries);
    facet_args fa;
    fa.facets = facets;
    fa.h_rows = facet_counts;
    ranked_extras x;
    x.fa = &fa;
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r, x,
                                          blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_faceted_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter,
                                    const dint_doc_facets* facets, size_t n_queries, uint64_t* counts, uint64_t* matches, float* scores,
                                    uint32_t* docids, uint32_t* facet_counts, uint64_t* blocks_decoded, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) ||
        !faceted_args_ok(qi, filter, facets, n_queries, facet_counts))
        return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(filter, nullptr, n_queries);
    facet_args fa;
    fa.facets = facets;
    fa.h_rows = facet_counts;
    ranked_extras x;
    x.fa = &fa;
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r, x,
                                          blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}
