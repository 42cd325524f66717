// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the BM25 maxima of the wand data built
// from the index on the device (wand_data.hpp:18-57 without the collection: DESIGN.md 4d-wand), and the block maxima of a wand handle.
// ---- maxima from the index ----------------------------------------------------------------------
// Every block of the index is decoded once, docs and freqs, in passes of consecutive blocks of at most
// DINT_OPT_QUERY_OR_PASS_PAGES pages (a list may span passes) through gather_decode_pages into the handle's probe / fprobe
// workspaces; block_max_weight_kernel leaves one float per block behind every pass. Then ONE list_max_weight_kernel over
// every list's block range. Nothing is waited for between the passes (no pass stages anything); both arrays come back in one
// copy at the end, through the handle's pinned staging area.

int dint_index_max_weights(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, float* max_term_weight,
                           float* block_max_weight, void* stream) {
    if (!qi || !freqs_dict || !wd) return DINT_ERR_ARG;
    const size_t n_lists = qi->list_len.size(), n_blocks = qi->n_blocks;
    if (n_lists && !max_term_weight) return DINT_ERR_ARG;
    if (freqs_dict->device != qi->docs->device || freqs_dict->kind != qi->docs->kind || wd->device != qi->docs->device) return DINT_ERR_ARG;
    if (qi->doc_bound > wd->num_docs) return DINT_ERR_ARG;  // (norm_lens[docid] must exist for every docID of the index)
    if (n_blocks == 0) {
        std::fill(max_term_weight, max_term_weight + n_lists, 0.0f);
        return DINT_OK;
    }
    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // results: block maxima [0, n_blocks), term maxima behind them; inputs: list_first
    const size_t n_out = n_blocks + n_lists;
    if (qi->stage(std::max(n_out, n_lists + 1) * 4) != hipSuccess || !qi->slot_score.ensure(n_out) || !qi->inputs.ensure(n_lists + 1))
        return DINT_ERR_HIP;
    float* const d_block_max = qi->slot_score.p;
    float* const d_term_max = qi->slot_score.p + n_blocks;
    std::copy(qi->list_first.begin(), qi->list_first.end(), qi->h(0));
    HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, (n_lists + 1) * 4, hipMemcpyHostToDevice, s));
    const uint32_t tb = 256;
    const size_t limit = size_t(std::min<long long>(opt(DINT_OPT_QUERY_OR_PASS_PAGES), 0x7FFFFFFFll));
    for (size_t b0 = 0; b0 != n_blocks;) {
        const size_t n = std::min(limit, n_blocks - b0);
        if (!qi->sub.ensure(n) || !qi->probe.ensure(n * kPageSlots) || !qi->fprobe.ensure(n * kPageSlots) || !qi->ms_touched.ensure(n))
            return stream_failed(s, DINT_ERR_HIP);
        hipLaunchKernelGGL(block_ids_kernel, dim3(uint32_t((n + tb - 1) / tb)), dim3(tb), 0, s, uint32_t(b0), uint32_t(n), qi->ms_touched.p);
        const int st = gather_decode_pages(qi, qi->ms_touched.p, nullptr, n, 0, freqs_dict, s);
        if (st != DINT_OK) return stream_failed(s, st);
        hipLaunchKernelGGL(block_max_weight_kernel, dim3(uint32_t(n)), dim3(kPageSlots), 0, s, qi->d_blocks, uint32_t(b0), qi->probe.p,
                           qi->fprobe.p, wd->d_norm_lens, d_block_max);
        if (hipGetLastError() != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
        b0 += n;
    }
    if (n_lists) {
        const uint32_t lists_per_group = tb / kWave;
        hipLaunchKernelGGL(list_max_weight_kernel, dim3(uint32_t((n_lists + lists_per_group - 1) / lists_per_group)), dim3(tb), 0, s,
                           qi->inputs.p, uint32_t(n_lists), d_block_max, d_term_max);
        if (hipGetLastError() != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
    }
    // (the list_first copy precedes this one on the stream: the staging area is free)
    float* const from = block_max_weight ? d_block_max : d_term_max;
    const size_t n_back = block_max_weight ? n_out : n_lists;
    if (n_back) HIP_TRY(hipMemcpyAsync(qi->h_stage, from, n_back * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const float* h = qi->h<float>(0);
    if (block_max_weight) {
        std::copy(h, h + n_blocks, block_max_weight);
        h += n_blocks;
    }
    std::copy(h, h + n_lists, max_term_weight);
    return DINT_OK;
}

// ---- block maxima of a wand handle --------------------------------------------------------------
int dint_wand_data_set_block_max_weights(dint_wand_data* wd, const float* block_max_weight, size_t n_blocks) {
    if (!wd || (n_blocks && !block_max_weight)) return DINT_ERR_ARG;
    // (the rule of dint_wand_data_create_with_max_weights: a NaN or negative maximum is refused, +inf is a legal upper bound)
    for (size_t b = 0; b != n_blocks; ++b)
        if (!(block_max_weight[b] >= 0.0f)) return DINT_ERR_ARG;
    HIP_TRY(hipSetDevice(wd->device));
    float* d = nullptr;
    if (n_blocks) {
        if (!hip_ok(counted_malloc(&d, n_blocks * sizeof(float)), "counted_malloc(block_max_weight)")) return DINT_ERR_HIP;
        if (!hip_ok(hipMemcpy(d, block_max_weight, n_blocks * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(block_max_weight)")) {
            (void)hipFree(d);
            return DINT_ERR_HIP;
        }
    }
    if (wd->d_block_max_weight) (void)hipFree(wd->d_block_max_weight);
    wd->d_block_max_weight = d;
    wd->n_block_max = n_blocks;
    wd->has_block_max = true;
    return DINT_OK;
}
