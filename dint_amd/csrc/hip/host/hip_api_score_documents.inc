// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": BM25 scores and term frequencies of
// caller-given documents (next_geq + freq, dict_posting_list.hpp:126-169, with ranked_or_query's sums: DESIGN.md 4d-score).
// ---- scores of given documents ------------------------------------------------------------------
// The plan is the queries' own (distinct terms with multiplicities). A query's host-known bound is sum_t min(blocks_t, its
// documents): a document claims at most one block of a term. A call is cut into passes of whole queries of at most
// DINT_OPT_QUERY_OR_PASS_PAGES of that bound (a larger query alone). Per pass:
//   in      one pinned copy: the term records, the queries, the documents
//   claims  sd_claim_kernel: per (document, term record) the block the docID falls in, once per (record, block)
//   decode  the touched blocks' docs and freqs parts, launches sized by the bound (the pages past the touched ones are empty)
//   score   sd_score_kernel: a thread per document
// The scores, the freqs matrices and every pass's touched count stay on the device and come back once, at the end.

namespace {
constexpr uint64_t kSdPassFlags = uint64_t(1) << 26;  // claim flags of a pass (a flag per block of every term record), 256 MiB
constexpr uint64_t kSdPassDocs = uint64_t(1) << 30;   // documents of a pass: a thread each, indexed in 32 bits
}  // namespace

int dint_score_documents(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, const uint32_t* terms,
                         const uint64_t* query_offsets, size_t n_queries, const uint32_t* docids, const uint64_t* doc_offsets,
                         float* scores, uint32_t* freqs, uint64_t* blocks_read, void* stream) {
    if (!qi || !freqs_dict || !wd || !scores) return DINT_ERR_ARG;
    if (n_queries && (!query_offsets || !doc_offsets)) return DINT_ERR_ARG;
    if (n_queries >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    for (size_t q = 0; q != n_queries; ++q)
        if (doc_offsets[q + 1] < doc_offsets[q] || doc_offsets[q + 1] - doc_offsets[q] > kSdPassDocs) return DINT_ERR_ARG;
    const uint64_t d_first = n_queries ? doc_offsets[0] : 0, d_all = n_queries ? doc_offsets[n_queries] - d_first : 0;
    if (d_all && !docids) return DINT_ERR_ARG;
    if (freqs_dict->device != qi->docs->device || freqs_dict->kind != qi->docs->kind || wd->device != qi->docs->device) return DINT_ERR_ARG;
    if (qi->doc_bound > wd->num_docs) return DINT_ERR_ARG;  // (norm_lens[docid] must exist for every docID of the index)
    if (blocks_read) *blocks_read = 0;
    if (n_queries == 0) return DINT_OK;
    query_plan plan;  // (with multiplicities; with_freqs: a query of one list is planned like any other)
    std::vector<uint64_t> unused(n_queries);
    const int planned = plan_queries(qi, terms, query_offsets, n_queries, true, true, true, unused.data(), nullptr, plan);
    if (planned != DINT_OK) return planned;
    if (d_all == 0) return DINT_OK;
    auto list_blocks = [&](uint32_t l) { return uint64_t(qi->list_first[l + 1] - qi->list_first[l]); };
    auto docs_of = [&](size_t q) { return doc_offsets[q + 1] - doc_offsets[q]; };
    // per query: its bound, its claim flags, where its freqs matrix begins; the passes
    std::vector<uint64_t> bound(n_queries, 0), flags(n_queries, 0), freq_at(n_queries + 1, 0);
    for (size_t q = 0; q != n_queries; ++q) {
        if (docs_of(q) != 0)
            for (uint32_t j = 0; j != plan.len[q]; ++j) {
                const uint64_t nb = list_blocks(plan.of(q)[j]);
                bound[q] += std::min<uint64_t>(nb, docs_of(q));
                flags[q] += nb;
            }
        freq_at[q + 1] = freq_at[q] + docs_of(q) * plan.len[q];
    }
    const uint64_t limit = uint64_t(opt(DINT_OPT_QUERY_OR_PASS_PAGES));
    std::vector<size_t> pass_first(1, 0);
    uint64_t in_pass = 0, in_flags = 0, in_docs = 0;
    for (size_t q = 0; q != n_queries; ++q) {
        if (docs_of(q) == 0) continue;
        if ((in_pass != 0 && in_pass + bound[q] > limit) || (in_flags != 0 && in_flags + flags[q] > kSdPassFlags) ||
            (in_docs != 0 && in_docs + docs_of(q) > kSdPassDocs)) {
            pass_first.push_back(q);
            in_pass = in_flags = in_docs = 0;
        }
        in_pass += bound[q];
        in_flags += flags[q];
        in_docs += docs_of(q);
    }
    pass_first.push_back(n_queries);
    // (a pass indexes its flags and pages in 32 bits: a query's distinct terms have at most the index's blocks, < 2^32 - 1)
    const size_t n_passes = pass_first.size() - 1;

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    auto failed = [&](int st) {
        (void)hipStreamSynchronize(s);
        return st;
    };
    // the call's results: a score per document, the freqs matrices back to back, a touched count per pass
    const uint64_t n_freqs = freqs ? freq_at[n_queries] : 0;
    if (!qi->slot_score.ensure(d_all) || !qi->target.ensure(std::max<uint64_t>(1, n_freqs)) || !qi->ms_count.ensure(n_passes))
        return DINT_ERR_HIP;
    HIP_TRY(hipMemsetAsync(qi->ms_count.p, 0, n_passes * 4, s));
    const uint32_t tb = 256;
    for (size_t k = 0; k != n_passes; ++k) {
        const size_t q0 = pass_first[k], q1 = pass_first[k + 1], nq = q1 - q0;
        const uint64_t doc0 = doc_offsets[q0] - d_first, n_docs = doc_offsets[q1] - doc_offsets[q0];
        if (n_docs == 0) continue;
        uint64_t n_rec = 0, B = 0, F = 0;
        uint32_t most_terms = 0;
        for (size_t q = q0; q != q1; ++q) {
            n_rec += plan.len[q];
            B += bound[q];
            F += flags[q];
            if (docs_of(q) != 0) most_terms = std::max(most_terms, plan.len[q]);
        }
        // inputs: per record {first, blocks, flag, q_weight, order}, per query {from, n}, per document {query, docID}, then
        // (8-byte aligned) per query where its freqs matrix begins, less the rows of the pass's documents before its own
        const size_t w_rec = 5 * n_rec, w_q = 2 * nq, u64_at = (w_rec + w_q + 2 * size_t(n_docs) + 1) / 2 * 2;
        const size_t words = u64_at + 2 * nq;
        if (k != 0) HIP_TRY(hipStreamSynchronize(s));  // (the last pass's inputs have left the staging area)
        if (qi->stage(words * 4) != hipSuccess) return failed(DINT_ERR_HIP);
        uint32_t* const h = static_cast<uint32_t*>(qi->h_stage);
        uint32_t *h_first = h, *h_blocks = h + n_rec, *h_flag = h_blocks + n_rec, *h_order = h_flag + 2 * n_rec;
        float* const h_weight = reinterpret_cast<float*>(h_flag + n_rec);
        uint32_t *h_qfrom = h + w_rec, *h_qn = h_qfrom + nq, *h_dq = h + w_rec + w_q, *h_did = h_dq + n_docs;
        uint64_t* const h_freq_at = reinterpret_cast<uint64_t*>(h + u64_at);
        uint32_t rec = 0, flag = 0;
        uint64_t doc = 0;
        for (size_t q = q0; q != q1; ++q) {
            const uint32_t from = rec, n = plan.len[q];
            const uint32_t* t = plan.of(q);
            h_qfrom[q - q0] = from;
            h_qn[q - q0] = n;
            h_freq_at[q - q0] = freq_at[q] - doc * n;  // (mod 2^64: the kernel adds the document's place in the pass times n)
            for (uint32_t j = 0; j != n; ++j, ++rec) {
                h_first[rec] = qi->list_first[t[j]];
                h_blocks[rec] = uint32_t(list_blocks(t[j]));
                h_flag[rec] = flag;
                h_weight[rec] = bm25_query_term_weight(plan.qf_of(q)[j], qi->list_len[t[j]], wd->num_docs);
                h_order[rec] = rec;
                if (docs_of(q) != 0) flag += h_blocks[rec];
            }
            // the query's records by ascending term id: the order its scores are summed in
            std::sort(h_order + from, h_order + from + n, [&](uint32_t a, uint32_t b) { return t[a - from] < t[b - from]; });
            for (uint64_t i = 0; i != docs_of(q); ++i, ++doc) h_dq[doc] = uint32_t(q - q0);
        }
        std::memcpy(h_did, docids + doc_offsets[q0], n_docs * 4);
        if (!qi->inputs.ensure(words) || !qi->ms_flag.ensure(std::max<uint64_t>(1, F)) || !qi->ms_rank.ensure(std::max<uint64_t>(1, F)) ||
            !qi->ms_touched.ensure(std::max<uint64_t>(1, B)))
            return failed(DINT_ERR_HIP);
        uint32_t* const d_in = qi->inputs.p;
        HIP_TRY(hipMemcpyAsync(d_in, h, words * 4, hipMemcpyHostToDevice, s));
        score_documents_pass sp{};
        sp.term_first = d_in;
        sp.term_blocks = d_in + n_rec;
        sp.term_flag = d_in + 2 * n_rec;
        sp.term_weight = reinterpret_cast<const float*>(d_in + 3 * n_rec);
        sp.term_order = d_in + 4 * n_rec;
        sp.q_from = d_in + w_rec;
        sp.q_n = sp.q_from + nq;
        sp.doc_query = d_in + w_rec + w_q;
        sp.doc_id = sp.doc_query + n_docs;
        sp.q_freq_at = reinterpret_cast<const uint64_t*>(d_in + u64_at);
        sp.n_docs = uint32_t(n_docs);
        sp.blocks = qi->d_blocks;
        sp.block_max = qi->d_block_max;
        sp.flag = qi->ms_flag.p;
        sp.rank = qi->ms_rank.p;
        sp.touched = qi->ms_touched.p;
        sp.n_touched = qi->ms_count.p + k;
        sp.norm_lens = wd->d_norm_lens;
        sp.score_out = qi->slot_score.p + doc0;
        sp.freqs_out = freqs ? qi->target.p : nullptr;
        const uint32_t grid = uint32_t((n_docs + tb - 1) / tb);
        if (B != 0) {
            if (!qi->sub.ensure(B) || !qi->probe.ensure(B * kPageSlots) || !qi->fprobe.ensure(B * kPageSlots)) return failed(DINT_ERR_HIP);
            HIP_TRY(hipMemsetAsync(qi->ms_flag.p, 0, F * 4, s));
            hipLaunchKernelGGL(sd_claim_kernel, dim3(grid, std::min<uint32_t>(most_terms, 1024)), dim3(tb), 0, s, sp);
            hipLaunchKernelGGL(gather_pages_kernel, dim3(uint32_t((B + tb - 1) / tb)), dim3(tb), 0, s, qi->d_blocks, qi->ms_touched.p, B,
                               qi->sub.p, static_cast<const uint32_t*>(sp.n_touched));
            const int st = decode_pages(qi, B, qi->probe.p, freqs_dict, qi->fprobe.p, s);
            if (st != DINT_OK) return failed(st);
        }
        sp.docs = qi->probe.p;
        sp.freqs = qi->fprobe.p;
        hipLaunchKernelGGL(sd_score_kernel, dim3(grid), dim3(tb), 0, s, sp);
        if (hipGetLastError() != hipSuccess) return failed(DINT_ERR_HIP);
    }
    std::vector<uint32_t> touched(n_passes, 0);
    HIP_TRY(hipMemcpyAsync(scores + d_first, qi->slot_score.p, d_all * sizeof(float), hipMemcpyDeviceToHost, s));
    if (n_freqs) HIP_TRY(hipMemcpyAsync(freqs, qi->target.p, n_freqs * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(touched.data(), qi->ms_count.p, n_passes * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (blocks_read)
        for (uint32_t n : touched) *blocks_read += n;
    return DINT_OK;
}
