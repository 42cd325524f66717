// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": document filters and the ranked
// queries under one (ranked_or_query / ranked_and_query, queries.hpp:309-457, over the documents of a bitmap).
// ---- document-filter ranked queries ---------------------------------------------------------------
// A filtered call is the unfiltered call (or_queries_impl / and_queries_impl with rk) with a filter_args threaded through it
// (DESIGN.md 4d-filter): the host plans only the LIVE blocks — those whose [base, max] holds a document of the filter, found
// once per filter on the device (dint_doc_filter_kernels.hpp) — and a kernel of that header retires what the live blocks
// hold outside the filter — OR: ranked_or_filtered_score_kernel in place of ranked_or_score_kernel; AND: filter_kill_kernel
// between the candidates' decode and the first round's search. The query weights come from the whole lists' lengths, so a
// match scores what the unfiltered call gives it. The selection, the workspaces and the lock are the unfiltered calls' own.

void dint_doc_filter_destroy(dint_doc_filter* f) {
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->d_bits) (void)hipFree(f->d_bits);
    if (f->d_live_before) (void)hipFree(f->d_live_before);
    delete f;
}

namespace {
// the workgroups of a scan over n elements (at least one: the partials are never empty)
uint32_t scan_grid(uint64_t n) { return uint32_t(std::max<uint64_t>(1, (n + kScanThreads - 1) / kScanThreads)); }

// out[0 .. n] <- the exclusive prefix sums whose workgroup level has just been launched on s (out[i]: within its
// workgroup; partials[g]: the workgroups' sums): the grid level and the add.
void scan_finish(uint32_t* out, uint64_t n, uint32_t* partials, hipStream_t s) {
    const uint32_t grid = scan_grid(n);
    hipLaunchKernelGGL(scan_partials_kernel, dim3(1), dim3(kScanThreads), 0, s, partials, uint64_t(grid), out + n);
    hipLaunchKernelGGL(scan_add_kernel, dim3(grid), dim3(kScanThreads), 0, s, out, n, partials);
}
}  // namespace

// A filter handle of num_docs documents for qi, shared by its two creations (dint_doc_filter_create and, hip_api_doc_values.inc,
// dint_doc_filter_create_from_values): fill(d_bits, n_words) puts the bitmap into the handle's own words on the device, masked
// at num_docs — an upload or a kernel on the null stream, under the index's lock — and the same rank-directory, liveness and
// scan launches follow.
static int doc_filter_build(dint_query_index* qi, uint64_t num_docs, const std::function<bool(uint64_t*, uint64_t)>& fill,
                            dint_doc_filter** out) {
    auto* f = new (std::nothrow) dint_doc_filter();
    if (!f) return DINT_ERR_NOMEM;
    f->qi = qi;
    f->device = qi->device;
    f->num_docs = num_docs;
    f->n_blocks = qi->n_blocks;
    const uint64_t n_words = (num_docs + 63) / 64, n_blocks = qi->n_blocks;
    try {
        f->live.assign(n_blocks, 0);
        f->live_before.assign(n_blocks + 1, 0u);
    } catch (const std::bad_alloc&) {
        delete f;
        return DINT_ERR_NOMEM;
    }

    std::lock_guard<std::mutex> lock(qi->mutex);
    // the creation's own memory: the rank directory (an entry per word and the total), the partials of either scan, the flags
    uint32_t *d_rank = nullptr, *d_partials = nullptr;
    uint8_t* d_live = nullptr;
    const uint64_t n_partials = std::max<uint64_t>(scan_grid(n_words), scan_grid(n_blocks));
    bool ok = hip_ok(hipSetDevice(qi->device), "hipSetDevice") &&
              hip_ok(counted_malloc(&f->d_bits, std::max<uint64_t>(1, n_words) * 8), "counted_malloc(filter bits)") &&
              hip_ok(counted_malloc(&f->d_live_before, (n_blocks + 1) * 4), "counted_malloc(live_before)") &&
              hip_ok(counted_malloc(&d_rank, (n_words + 1) * 4), "counted_malloc(filter rank)") &&
              hip_ok(counted_malloc(&d_partials, n_partials * 4), "counted_malloc(filter partials)") &&
              hip_ok(counted_malloc(&d_live, std::max<uint64_t>(1, n_blocks)), "counted_malloc(filter live)") &&
              (n_words == 0 || fill(f->d_bits, n_words));
    uint32_t n_set = 0;
    if (ok) {
        hipStream_t s = nullptr;
        // 1. the rank directory
        hipLaunchKernelGGL(filter_word_rank_kernel, dim3(scan_grid(n_words)), dim3(kScanThreads), 0, s, f->d_bits, n_words, d_rank, d_partials);
        scan_finish(d_rank, n_words, d_partials, s);
        // 2. block liveness and 3. the live rank (the stream orders the partials' second use behind their first)
        hipLaunchKernelGGL(filter_block_live_kernel, dim3(scan_grid(n_blocks)), dim3(kScanThreads), 0, s, qi->d_blocks, n_blocks, f->d_bits,
                           d_rank, uint32_t(num_docs), d_live, f->d_live_before, d_partials);
        scan_finish(f->d_live_before, n_blocks, d_partials, s);
        ok = hip_ok(hipGetLastError(), "doc filter kernels") &&
             hip_ok(hipMemcpy(&n_set, d_rank + n_words, 4, hipMemcpyDeviceToHost), "hipMemcpy(n_set)") &&
             (n_blocks == 0 || hip_ok(hipMemcpy(f->live.data(), d_live, n_blocks, hipMemcpyDeviceToHost), "hipMemcpy(live)")) &&
             // (the host's live rank is the device's own, copied back: the planning counts a list's pages with it in O(1))
             hip_ok(hipMemcpy(f->live_before.data(), f->d_live_before, (n_blocks + 1) * 4, hipMemcpyDeviceToHost), "hipMemcpy(live_before)");
    }
    for (void* p : {static_cast<void*>(d_rank), static_cast<void*>(d_partials), static_cast<void*>(d_live)})
        if (p) (void)hipFree(p);
    if (!ok) {
        dint_doc_filter_destroy(f);
        return DINT_ERR_HIP;
    }
    f->n_set = n_set;
    *out = f;
    return DINT_OK;
}

int dint_doc_filter_create(dint_query_index* qi, const uint64_t* bits, uint64_t num_docs, dint_doc_filter** out) {
    if (!qi || !out || (num_docs && !bits) || num_docs > 0xFFFFFFFFull) return DINT_ERR_ARG;
    *out = nullptr;
    // the handle's own copy is the device's: the caller's words go there as they are, and the last word again, masked at num_docs
    return doc_filter_build(qi, num_docs, [&](uint64_t* d_bits, uint64_t n_words) {
        const uint64_t last_word = num_docs & 63u ? bits[n_words - 1] & ((1ull << (num_docs & 63u)) - 1ull) : bits[n_words - 1];
        return hip_ok(hipMemcpy(d_bits, bits, n_words * 8, hipMemcpyHostToDevice), "hipMemcpy(filter bits)") &&
               hip_ok(hipMemcpy(d_bits + (n_words - 1), &last_word, 8, hipMemcpyHostToDevice), "hipMemcpy(filter last word)");
    }, out);
}

int dint_doc_filter_info_get(const dint_doc_filter* f, dint_doc_filter_info* info) {
    if (!f || !info) return DINT_ERR_ARG;
    info->num_docs = f->num_docs;
    info->n_set = f->n_set;
    info->n_blocks = f->n_blocks;
    info->live_blocks = f->live_before[f->n_blocks];
    return DINT_OK;
}

int dint_ranked_or_filtered_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter, size_t n_queries,
                                    uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded,
                                    void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || (filter && filter->qi != qi)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(filter, nullptr, n_queries);  // (no filter: the ranged call on null ranges)
    const int st = ranked_restricted_call(false, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r,
                                          ranked_extras(), blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}

int dint_ranked_and_filtered_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                     const uint32_t* terms, const uint64_t* query_offsets, const dint_doc_filter* filter, size_t n_queries,
                                     uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded,
                                     void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores) || (filter && filter->qi != qi)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull), h_matches;
    restriction r(filter, nullptr, n_queries);  // (no filter: the ranged call on null ranges)
    const int st = ranked_restricted_call(true, qi, freqs_dict, ranked_args_of(wd, k, keys.data()), terms, query_offsets, n_queries, counts, r,
                                          ranked_extras(), blocks_decoded, h_matches, stream);
    if (st != DINT_OK) return st;
    restricted_outputs(keys, n_queries, k, h_matches, counts, matches, scores, docids);
    return DINT_OK;
}
