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
    // per query: its documents, its bound, its claim flags, where its freqs matrix begins; the passes
    std::vector<uint64_t> n_docs_of(n_queries, 0), bound(n_queries, 0), flags(n_queries, 0), freq_at(n_queries + 1, 0);
    for (size_t q = 0; q != n_queries; ++q) {
        n_docs_of[q] = doc_offsets[q + 1] - doc_offsets[q];
        if (n_docs_of[q] != 0)
            for (uint32_t j = 0; j != plan.len[q]; ++j) {
                const uint64_t nb = qi->blocks_of(plan.of(q)[j]);
                bound[q] += std::min<uint64_t>(nb, n_docs_of[q]);
                flags[q] += nb;
            }
        freq_at[q + 1] = freq_at[q] + n_docs_of[q] * plan.len[q];
    }
    const std::vector<size_t> pass_first = cut_passes(n_queries, {{bound.data(), uint64_t(opt(DINT_OPT_QUERY_OR_PASS_PAGES))},
                                                                  {flags.data(), kSdPassFlags}, {n_docs_of.data(), kSdPassDocs}}, true);
    // (a pass indexes its flags and pages in 32 bits: a query's distinct terms have at most the index's blocks, < 2^32 - 1)
    const size_t n_passes = pass_first.size() - 1;

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
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
            if (n_docs_of[q] != 0) most_terms = std::max(most_terms, plan.len[q]);
        }
        const score_documents_layout L(n_rec, nq, n_docs);
        if (k != 0) HIP_TRY(hipStreamSynchronize(s));  // (the last pass's inputs have left the staging area)
        if (qi->stage(L.words * 4) != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
        uint32_t *h_blocks = qi->h(L.term_blocks), *h_order = qi->h(L.term_order), *h_dq = qi->h(L.doc_query);
        uint32_t rec = 0, flag = 0;
        uint64_t doc = 0;
        for (size_t q = q0; q != q1; ++q) {
            const uint32_t from = rec, n = plan.len[q];
            const uint32_t* t = plan.of(q);
            qi->h(L.q_from)[q - q0] = from;
            qi->h(L.q_n)[q - q0] = n;
            qi->h<uint64_t>(L.q_freq_at)[q - q0] = freq_at[q] - doc * n;  // (mod 2^64: the kernel adds the document's place in the pass times n)
            for (uint32_t j = 0; j != n; ++j, ++rec) {
                qi->h(L.term_first)[rec] = qi->list_first[t[j]];
                h_blocks[rec] = qi->blocks_of(t[j]);
                qi->h(L.term_flag)[rec] = flag;
                qi->h<float>(L.term_weight)[rec] = bm25_query_term_weight(plan.qf_of(q)[j], qi->list_len[t[j]], wd->num_docs);
                if (n_docs_of[q] != 0) flag += h_blocks[rec];
            }
            sort_records_by_term(h_order, from, n, t);
            for (uint64_t i = 0; i != n_docs_of[q]; ++i, ++doc) h_dq[doc] = uint32_t(q - q0);
        }
        std::memcpy(qi->h(L.doc_id), docids + doc_offsets[q0], n_docs * 4);
        if (!qi->inputs.ensure(L.words) || !qi->ms_flag.ensure(std::max<uint64_t>(1, F)) || !qi->ms_rank.ensure(std::max<uint64_t>(1, F)) ||
            !qi->ms_touched.ensure(std::max<uint64_t>(1, B)))
            return stream_failed(s, DINT_ERR_HIP);
        HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, L.words * 4, hipMemcpyHostToDevice, s));
        score_documents_pass sp{};
        sp.term_first = qi->d(L.term_first);
        sp.term_blocks = qi->d(L.term_blocks);
        sp.term_flag = qi->d(L.term_flag);
        sp.term_weight = qi->d<const float>(L.term_weight);
        sp.term_order = qi->d(L.term_order);
        sp.q_from = qi->d(L.q_from);
        sp.q_n = qi->d(L.q_n);
        sp.doc_query = qi->d(L.doc_query);
        sp.doc_id = qi->d(L.doc_id);
        sp.q_freq_at = qi->d<const uint64_t>(L.q_freq_at);
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
            if (!qi->sub.ensure(B) || !qi->probe.ensure(B * kPageSlots) || !qi->fprobe.ensure(B * kPageSlots)) return stream_failed(s, DINT_ERR_HIP);
            HIP_TRY(hipMemsetAsync(qi->ms_flag.p, 0, F * 4, s));
            hipLaunchKernelGGL(sd_claim_kernel, dim3(grid, std::min<uint32_t>(most_terms, 1024)), dim3(tb), 0, s, sp);
            const int st = gather_decode_pages(qi, qi->ms_touched.p, sp.n_touched, B, 0, freqs_dict, s);
            if (st != DINT_OK) return stream_failed(s, st);
        }
        sp.docs = qi->probe.p;
        sp.freqs = qi->fprobe.p;
        hipLaunchKernelGGL(sd_score_kernel, dim3(grid), dim3(tb), 0, s, sp);
        if (hipGetLastError() != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
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
