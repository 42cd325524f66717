// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": ranked conjunctive queries
// (ranked_and_query, queries.hpp:309-385) and the wand data they read (wand_data.hpp:18-57).
// ---- ranked conjunctive queries -----------------------------------------------------------------
// A ranked call is an and_query<true> call (and_queries_impl) whose freqs pass scores instead of summing: per term, in
// the AND path's order, ranked_gather_kernel adds q_weight * doc_term_weight to every match's slot. Behind the last term,
// ranked_topk selects the k best of every query (dint_ranked_query_kernels.hpp). The claim tables, workspaces and lock
// are the AND calls' own.

struct dint_wand_data {
    int device = 0;
    uint64_t num_docs = 0;
    float* d_norm_lens = nullptr;
    // dint_wand_data_create_with_max_weights: max_term_weight[n_lists], on the host (only the pruned ranked call reads it)
    bool has_max_weights = false;
    std::vector<float> max_term_weight;
    // dint_wand_data_set_block_max_weights (hip_api_wand.inc): a maximum per block of a query index, on the device
    bool has_block_max = false;
    size_t n_block_max = 0;
    float* d_block_max_weight = nullptr;
};

void dint_wand_data_destroy(dint_wand_data* wd) {
    if (!wd) return;
    (void)hipSetDevice(wd->device);
    if (wd->d_norm_lens) (void)hipFree(wd->d_norm_lens);
    if (wd->d_block_max_weight) (void)hipFree(wd->d_block_max_weight);
    delete wd;
}

int dint_wand_data_create(int device, const float* norm_lens, uint64_t num_docs, dint_wand_data** out) {
    if (!out || (num_docs && !norm_lens) || num_docs > 0x100000000ull) return DINT_ERR_ARG;
    *out = nullptr;
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) return DINT_ERR_NO_DEVICE;
    auto* wd = new (std::nothrow) dint_wand_data();
    if (!wd) return DINT_ERR_NOMEM;
    wd->device = device;
    wd->num_docs = num_docs;
    const bool ok = hip_ok(hipSetDevice(device), "hipSetDevice") &&
                    hip_ok(counted_malloc(&wd->d_norm_lens, std::max<uint64_t>(1, num_docs) * sizeof(float)), "counted_malloc(norm_lens)") &&
                    (num_docs == 0 ||
                     hip_ok(hipMemcpy(wd->d_norm_lens, norm_lens, num_docs * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(norm_lens)"));
    if (!ok) {
        dint_wand_data_destroy(wd);
        return DINT_ERR_HIP;
    }
    *out = wd;
    return DINT_OK;
}

int dint_wand_data_create_with_max_weights(int device, const float* norm_lens, uint64_t num_docs, const float* max_term_weight,
                                           size_t n_lists, dint_wand_data** out) {
    if (!out || (n_lists && !max_term_weight)) return DINT_ERR_ARG;
    *out = nullptr;
    // a NaN or negative maximum is refused: the pruned call orders a query's terms by q_weight * maximum, and a NaN there
    // is no strict weak ordering for std::sort (+inf is a legal upper bound: its term is never left out)
    for (size_t t = 0; t != n_lists; ++t)
        if (!(max_term_weight[t] >= 0.0f)) return DINT_ERR_ARG;
    const int st = dint_wand_data_create(device, norm_lens, num_docs, out);
    if (st != DINT_OK) return st;
    dint_wand_data* wd = *out;
    try {
        wd->max_term_weight.assign(max_term_weight, max_term_weight + n_lists);
    } catch (const std::bad_alloc&) {
        dint_wand_data_destroy(wd);
        *out = nullptr;
        return DINT_ERR_NOMEM;
    }
    wd->has_max_weights = true;
    return DINT_OK;
}

// The selection of and_queries_impl's ranked form, on its stream, behind the freqs pass: query q's candidate pages are the
// pages p with page_query[p] == q (consecutive). Its slots are cut into runs of R keys, every run sorted, then the runs
// merged pairwise, pass after pass (a pass serves every query of the call), until run 0 of every query holds its best R.
// rk.keys <- the first k of them (copied on the stream: the caller synchronises). sv (a sorted call): the runs are sorted by
// the key of the column's value (topk_sort_runs_by_value_kernel); the merges and the output order whatever keys they get.
static int ranked_topk(dint_query_index* qi, const ranked_args& rk, const std::vector<uint32_t>& page_query, size_t n_queries,
                       hipStream_t s, const sort_args* sv) {
    uint32_t R = kPageSlots;
    while (R < rk.k) R <<= 1;
    // (the runs, the tasks and their tables, topk_layout, in pageable memory of this frame: hence the wait)
    const topk_runs runs(page_query, n_queries, kPageSlots, R);
    const std::vector<size_t>& pass_first = runs.pass_first;
    const uint64_t n_keys = runs.n_keys;
    const topk_layout L(runs.tasks.size(), n_queries);
    const std::vector<uint32_t> h = runs.words(L);
    if (!qi->topk_in.ensure(L.words) || !qi->topk_keys.ensure(std::max<uint64_t>(1, n_keys)) ||
        !qi->topk_out.ensure(uint64_t(n_queries) * rk.k))
        return DINT_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(qi->topk_in.p, h.data(), L.words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    const topk_task* const d_tasks = staged<const topk_task>(qi->topk_in.p, L.tasks);
    const uint32_t* const d_page_first = staged(qi->topk_in.p, L.page_first);
    const uint32_t* const d_pages = staged(qi->topk_in.p, L.pages);
    const unsigned long long* const d_base = staged<const unsigned long long>(qi->topk_in.p, L.key_base);
    const uint32_t tb = 256;
    for (size_t p = 0; p + 1 < pass_first.size(); ++p) {
        const size_t n_tasks = pass_first[p + 1] - pass_first[p];
        if (n_tasks == 0) continue;
        if (p == 0 && sv)
            hipLaunchKernelGGL(topk_sort_runs_by_value_kernel, dim3(uint32_t(n_tasks)), dim3(tb), R * sizeof(unsigned long long), s, d_tasks,
                               d_page_first, d_pages, d_base, qi->cand.p, sv->values->view(), sv->order, R, qi->topk_keys.p);
        else if (p == 0)
            hipLaunchKernelGGL(topk_sort_runs_kernel, dim3(uint32_t(n_tasks)), dim3(tb), R * sizeof(unsigned long long), s, d_tasks,
                               d_page_first, d_pages, d_base, qi->cand.p, qi->slot_score.p, R, qi->topk_keys.p);
        else
            hipLaunchKernelGGL(topk_merge_kernel, dim3(uint32_t(n_tasks)), dim3(tb), R * sizeof(unsigned long long), s,
                               d_tasks + pass_first[p], d_base, R, qi->topk_keys.p);
    }
    const uint64_t n_out = uint64_t(n_queries) * rk.k;
    hipLaunchKernelGGL(topk_out_kernel, dim3(uint32_t((n_out + tb - 1) / tb)), dim3(tb), 0, s, d_base, d_pages, qi->topk_keys.p,
                       uint32_t(n_queries), rk.k, qi->topk_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rk.keys, qi->topk_out.p, n_out * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// Both ranked entries' own checks (null handles and a bad k are refused before anything is dereferenced)
static bool ranked_args_ok(const dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                           const uint64_t* query_offsets, size_t n_queries, const uint64_t* counts, const float* scores) {
    if (!qi || !freqs_dict || !wd || k == 0 || k > kRankedMaxK) return false;
    if (n_queries && (!query_offsets || !counts || !scores)) return false;
    if (freqs_dict->device != qi->docs->device || freqs_dict->kind != qi->docs->kind || wd->device != qi->docs->device) return false;
    if (qi->doc_bound > wd->num_docs) return false;  // (norm_lens[docid] must exist for every docID of the index)
    return n_queries < 0xFFFFFFFFull && uint64_t(n_queries) * k <= (uint64_t(1) << 32);
}

// what a ranked call scores with, from the wand handle; keys: where the selection goes
static ranked_args ranked_args_of(const dint_wand_data* wd, uint32_t k, unsigned long long* keys) {
    return ranked_args{wd->d_norm_lens, k, keys, wd->num_docs};
}

// the ranked OR calls' counts: every score is > 0, so a query's keys are non-zero for its first min(k, |union|) and zero past them
static void counts_from_keys(const std::vector<unsigned long long>& keys, size_t n_queries, uint32_t k, uint64_t* counts) {
    for (size_t q = 0; q != n_queries; ++q) {
        uint64_t c = 0;
        while (c != k && keys[q * k + c] != 0) ++c;
        counts[q] = c;
    }
}

// ranked_topk's keys (score bits, then the inverted docID; sorted descending) -> the first counts[q] scores and docIDs of
// every query, 0.0f and 0xFFFFFFFF past them
static void unpack_keys(const std::vector<unsigned long long>& keys, size_t n_queries, uint32_t k, const uint64_t* counts,
                        float* scores, uint32_t* docids) {
    for (size_t q = 0; q != n_queries; ++q)
        for (uint32_t i = 0; i != k; ++i) {
            const unsigned long long key = i < counts[q] ? keys[q * k + i] : 0ull;
            const uint32_t bits = uint32_t(key >> 32);
            float sc = 0.0f;
            std::memcpy(&sc, &bits, 4);
            scores[q * k + i] = key ? sc : 0.0f;
            if (docids) docids[q * k + i] = key ? 0xFFFFFFFFu - uint32_t(key) : 0xFFFFFFFFu;
        }
}

int dint_ranked_and_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                            const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts, float* scores,
                            uint32_t* docids, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    std::vector<uint64_t> freq_sums(n_queries, 0);
    const ranked_args rk = ranked_args_of(wd, k, keys.data());
    // (and_queries_impl checks the offsets and the terms before anything is launched)
    const int st = and_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums.data(), nullptr, stream, ranked_extras(),
                                    false, &rk);
    if (st != DINT_OK) return st;
    for (size_t q = 0; q != n_queries; ++q) counts[q] = std::min<uint64_t>(counts[q], k);
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
