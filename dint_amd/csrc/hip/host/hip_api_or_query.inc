// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": disjunctive queries (queries.hpp:86-130).
// ---- disjunctive queries ------------------------------------------------------------------------
// or_query visits every docID some list of the query holds, once, and (with_freqs) reads the freq of every posting: every
// block of every distinct term is decoded, so there is nothing to skip and nothing to claim. A call is cut into passes of
// whole queries of at most DINT_OPT_QUERY_OR_PASS_PAGES pages; per pass one copy in, the pages' decode (decode_pages, as
// the AND path decodes its freqs pages) and ONE probe launch (or_count_kernel, dint_or_query_kernels.hpp) that adds to the
// call's counters. The counters come back once, at the end. The claim flags and tables of the AND forms are not touched.
// rk (dint_ranked_or_queries, hip_api_ranked_or_query.inc): the pass's probe launch is ranked_or_score_kernel instead, and
// ranked_topk writes the best keys of the pass's queries to rk->keys at their own offset; the counters are not used.

// The set-up of an OR call, shared with the pruned ranked call (hip_api_ranked_or_maxscore.inc): the plan (longest list
// first, with multiplicities if with_qf), every query's pages (every block of its distinct terms; a query without any
// has len 0) and the passes: whole queries, at most `limit` pages each — a query larger than that alone, in a pass sized to it.
struct or_passes {
    query_plan plan;
    std::vector<uint64_t> pages;  // per query
    std::vector<size_t> first;    // pass k: queries [first[k], first[k + 1])
    uint64_t all = 0;
};
static int plan_or_passes(const dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                          bool with_qf, bool with_freqs, uint64_t* counts, uint64_t* freq_sums, or_passes& op) {
    query_plan& plan = op.plan;
    const int planned = plan_queries(qi, terms, query_offsets, n_queries, true, with_qf, with_freqs, counts, freq_sums, plan);
    if (planned != DINT_OK) return planned;
    op.pages.assign(n_queries, 0);
    op.all = 0;
    for (size_t q = 0; q != n_queries; ++q) {
        for (uint32_t j = 0; j != plan.len[q]; ++j) {
            const uint32_t l = plan.of(q)[j];
            op.pages[q] += qi->list_first[l + 1] - qi->list_first[l];
        }
        if (op.pages[q] == 0) plan.len[q] = 0;  // (lists without a block)
        op.all += op.pages[q];
    }
    const uint64_t limit = uint64_t(opt(DINT_OPT_QUERY_OR_PASS_PAGES));
    op.first.assign(1, 0);
    uint64_t in_pass = 0;
    for (size_t q = 0; q != n_queries; ++q) {
        if (in_pass != 0 && in_pass + op.pages[q] > limit) {
            op.first.push_back(q);
            in_pass = 0;
        }
        in_pass += op.pages[q];
    }
    op.first.push_back(n_queries);
    return DINT_OK;
}

static int or_queries_impl(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                           size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks, void* stream,
                           const ranked_args* rk = nullptr) {
    if (!qi || (n_queries && (!query_offsets || !counts))) return DINT_ERR_ARG;
    if (freq_blocks) *freq_blocks = 0;
    if (n_queries == 0) return DINT_OK;
    if (n_queries >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    or_passes op;  // (rk: with multiplicities, for the query weights)
    const int planned = plan_or_passes(qi, terms, query_offsets, n_queries, rk != nullptr, freqs_dict != nullptr, counts, freq_sums, op);
    if (planned != DINT_OK) return planned;
    const query_plan& plan = op.plan;
    const std::vector<uint64_t>& plan_pages = op.pages;
    const std::vector<size_t>& pass_first = op.first;
    auto list_blocks = [&](uint32_t l) { return uint64_t(qi->list_first[l + 1] - qi->list_first[l]); };
    if (op.all == 0) return DINT_OK;

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // the call's counters: counts[n_queries] then freq sums[n_queries], cleared once, added to by every pass
    if (!qi->freq_sums.ensure(2 * n_queries)) return DINT_ERR_HIP;
    unsigned long long* const d_counts = qi->freq_sums.p;
    unsigned long long* const d_sums = d_counts + n_queries;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * n_queries * sizeof(unsigned long long), s));
    auto failed = [&](int st) {
        (void)hipStreamSynchronize(s);
        return st;
    };
    for (size_t k = 0; k + 1 < pass_first.size(); ++k) {
        const size_t q0 = pass_first[k], q1 = pass_first[k + 1];
        uint64_t n_pages = 0, n_terms = 0;
        for (size_t q = q0; q != q1; ++q) {
            n_pages += plan_pages[q];
            n_terms += plan.len[q];
        }
        if (n_pages == 0) continue;
        // inputs: page -> block, page -> term record, then per term record {first block, blocks, first page, query, from}
        // (rk: and {the records of its query by term id, its query's terms, q_weight})
        const size_t words = 2 * n_pages + (rk ? 8 : 5) * n_terms;
        if (k != 0) HIP_TRY(hipStreamSynchronize(s));  // (the last pass's inputs have left the staging area)
        if (qi->stage(std::max<size_t>(words * 4, 2 * n_queries * sizeof(unsigned long long))) != hipSuccess) return failed(DINT_ERR_HIP);
        uint32_t* const h = static_cast<uint32_t*>(qi->h_stage);
        uint32_t *page_block = h, *page_term = h + n_pages, *term_first = h + 2 * n_pages, *term_blocks = term_first + n_terms,
                 *term_page = term_blocks + n_terms, *term_query = term_page + n_terms, *term_from = term_query + n_terms,
                 *term_order = term_from + n_terms, *term_n = term_order + n_terms;
        float* const term_weight = reinterpret_cast<float*>(term_n + n_terms);
        uint32_t page = 0, rec = 0;
        for (size_t q = q0; q != q1; ++q) {
            const uint32_t from = rec;
            if (rk) {  // the query's records by ascending term id: the order its scores are summed in
                for (uint32_t j = 0; j != plan.len[q]; ++j) term_order[from + j] = from + j;
                std::sort(term_order + from, term_order + from + plan.len[q],
                          [&](uint32_t a, uint32_t b) { return plan.of(q)[a - from] < plan.of(q)[b - from]; });
            }
            for (uint32_t j = 0; j != plan.len[q]; ++j, ++rec) {
                const uint32_t l = plan.of(q)[j];
                term_first[rec] = qi->list_first[l];
                term_blocks[rec] = uint32_t(list_blocks(l));
                term_page[rec] = page;
                term_query[rec] = uint32_t(q);
                term_from[rec] = from;
                if (rk) {
                    term_n[rec] = plan.len[q];
                    term_weight[rec] = bm25_query_term_weight(plan.qf_of(q)[j], qi->list_len[l], rk->num_docs);
                }
                for (uint32_t b = qi->list_first[l]; b != qi->list_first[l + 1]; ++b, ++page) {
                    page_block[page] = b;
                    page_term[page] = rec;
                }
            }
        }
        if (!qi->inputs.ensure(words) || !qi->sub.ensure(n_pages) || !qi->probe.ensure(n_pages * kPageSlots) ||
            (freqs_dict && !qi->fprobe.ensure(n_pages * kPageSlots)))
            return failed(DINT_ERR_HIP);
        uint32_t* const d_in = qi->inputs.p;
        HIP_TRY(hipMemcpyAsync(d_in, h, words * 4, hipMemcpyHostToDevice, s));
        const uint32_t tb = 256;
        hipLaunchKernelGGL(gather_pages_kernel, dim3(uint32_t((n_pages + tb - 1) / tb)), dim3(tb), 0, s, qi->d_blocks, d_in, n_pages,
                           qi->sub.p, static_cast<const uint32_t*>(nullptr));
        const int st = decode_pages(qi, n_pages, qi->probe.p, freqs_dict, freqs_dict ? qi->fprobe.p : nullptr, s);
        if (st != DINT_OK) return failed(st);
        or_pass p{};
        p.page_block = d_in;
        p.page_term = d_in + n_pages;
        p.term_first = d_in + 2 * n_pages;
        p.term_blocks = p.term_first + n_terms;
        p.term_page = p.term_blocks + n_terms;
        p.term_query = p.term_page + n_terms;
        p.term_from = p.term_query + n_terms;
        p.blocks = qi->d_blocks;
        p.block_max = qi->d_block_max;
        p.docs = qi->probe.p;
        p.freqs = freqs_dict ? qi->fprobe.p : nullptr;
        p.counts = d_counts;
        p.freq_sums = d_sums;
        if (rk) {  // score the union's representatives, then select every query's best k (one query: one pass)
            if (!qi->cand.ensure(n_pages * kPageSlots) || !qi->slot_score.ensure(n_pages * kPageSlots)) return failed(DINT_ERR_HIP);
            ranked_or_pass rp{};
            rp.base = p;
            rp.term_order = p.term_from + n_terms;
            rp.term_n = rp.term_order + n_terms;
            rp.term_weight = reinterpret_cast<const float*>(rp.term_n + n_terms);
            rp.norm_lens = rk->norm_lens;
            rp.cand = qi->cand.p;
            rp.score = qi->slot_score.p;
            hipLaunchKernelGGL(ranked_or_score_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, rp);
            if (hipGetLastError() != hipSuccess) return failed(DINT_ERR_HIP);
            std::vector<uint32_t> page_query(n_pages);  // (the pass's queries, from 0)
            for (uint64_t pg = 0; pg != n_pages; ++pg) page_query[pg] = term_query[page_term[pg]] - uint32_t(q0);
            ranked_args pass_rk = *rk;
            pass_rk.keys = rk->keys + uint64_t(q0) * rk->k;
            const int rst = ranked_topk(qi, pass_rk, page_query, q1 - q0, s);
            if (rst != DINT_OK) return failed(rst);
            continue;
        }
        hipLaunchKernelGGL(or_count_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, p);
        if (hipGetLastError() != hipSuccess) return failed(DINT_ERR_HIP);
    }
    HIP_TRY(hipStreamSynchronize(s));  // (the last pass's inputs have left the staging area: the results go there)
    if (rk) return DINT_OK;            // (ranked: the keys are already on the host)
    if (qi->stage(2 * n_queries * sizeof(unsigned long long)) != hipSuccess) return DINT_ERR_HIP;
    unsigned long long* const h_res = static_cast<unsigned long long*>(qi->h_stage);
    HIP_TRY(hipMemcpyAsync(h_res, d_counts, (freqs_dict ? 2 : 1) * n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t q = 0; q != n_queries; ++q)
        if (plan.len[q] != 0) {
            counts[q] = h_res[q];
            if (freqs_dict) {
                freq_sums[q] = h_res[n_queries + q];
                if (freq_blocks) *freq_blocks += plan_pages[q];
            }
        }
    return DINT_OK;
}

int dint_or_queries(dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                    uint64_t* counts, void* stream) {
    return or_queries_impl(qi, nullptr, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream);
}

int dint_or_queries_freqs(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                          size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks_decoded, void* stream) {
    if (!freqs_args_ok(qi, freqs_dict, freq_sums)) return DINT_ERR_ARG;
    return or_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums, freq_blocks_decoded, stream);
}
