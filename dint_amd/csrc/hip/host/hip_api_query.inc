// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the query index handle; the page decodes every query call is made of
// (the calls themselves: hip_api_query_plan.inc, hip_api_query_and.inc, hip_api_or_query.inc, hip_api_ranked*.inc, hip_api_score_documents.inc).
// ---- query index, page decodes ------------------------------------------------------------------

void dint_query_index_destroy(dint_query_index* qi) {
    if (!qi) return;
    (void)hipSetDevice(qi->device);  // (the workspaces are freed by delete, on this device; qi->docs may be gone already)
    for (void* p : {static_cast<void*>(qi->d_blocks), static_cast<void*>(qi->d_block_max), static_cast<void*>(qi->d_needed),
                    static_cast<void*>(qi->d_rank), static_cast<void*>(qi->d_touched)})
        if (p) (void)hipFree(p);
    if (qi->h_stage) (void)hipHostFree(qi->h_stage);
    for (void* p : qi->h_expect)
        if (p) (void)hipHostFree(p);
    delete qi;
}

int dint_query_index_create(const dint_dict* docs_dict, const uint8_t* d_index, size_t index_bytes,
                            const dint_block_ref* blocks, size_t n_blocks, size_t n_lists, dint_query_index** out) {
    if (!docs_dict || !out || (!blocks && n_blocks) || (!d_index && n_blocks)) return DINT_ERR_ARG;
    if (n_blocks >= 0xFFFFFFFFull || n_lists >= 0xFFFFFFFFull || (n_blocks && index_bytes < 8)) return DINT_ERR_ARG;
    *out = nullptr;
    auto* qi = new (std::nothrow) dint_query_index();
    if (!qi) return DINT_ERR_NOMEM;
    qi->docs = docs_dict;
    qi->device = docs_dict->device;
    qi->d_index = d_index;
    qi->index_bytes = index_bytes;
    qi->n_blocks = n_blocks;
    qi->list_first.assign(n_lists + 1, 0);
    qi->list_len.assign(n_lists, 0);
    std::vector<uint32_t>& maxs = qi->block_max;  // (kept: the ranged calls plan their pages on the host)
    maxs.assign(n_blocks, 0u);
    uint32_t prev_list = 0;
    for (size_t b = 0; b != n_blocks; ++b) {
        const uint32_t l = blocks[b].list;
        // lists in order, each list's blocks contiguous; docID 0xFFFFFFFF is kDeadCandidate, no docID (num_docs <= 2^32 - 1)
        if (l >= n_lists || l < prev_list || blocks[b].n == 0 || blocks[b].n > 256 || blocks[b].in_off > index_bytes ||
            blocks[b].max == 0xFFFFFFFFu) {
            delete qi;
            return DINT_ERR_FORMAT;
        }
        if (b != 0 && blocks[b - 1].list == l && blocks[b - 1].n != 256) qi->whole_blocks = false;
        prev_list = l;
        qi->list_first[l + 1] += 1;
        qi->list_len[l] += blocks[b].n;
        maxs[b] = blocks[b].max;
        qi->doc_bound = std::max<uint64_t>(qi->doc_bound, uint64_t(blocks[b].max) + 1);
    }
    for (size_t l = 0; l != n_lists; ++l) qi->list_first[l + 1] += qi->list_first[l];
    const size_t nb = std::max<size_t>(1, n_blocks);
    bool ok = hip_ok(hipSetDevice(docs_dict->device), "hipSetDevice") &&
              hip_ok(counted_malloc(&qi->d_blocks, nb * sizeof(dint_block_ref)), "counted_malloc(blocks)") &&
              hip_ok(counted_malloc(&qi->d_block_max, nb * 4), "counted_malloc(block_max)") &&
              hip_ok(counted_malloc(&qi->d_needed, 2 * nb * 4), "counted_malloc(needed)") &&  // (two sets of each: round_tail)
              hip_ok(counted_malloc(&qi->d_rank, 2 * nb * 4), "counted_malloc(rank)") &&
              hip_ok(counted_malloc(&qi->d_touched, 2 * nb * 4), "counted_malloc(touched)") &&
              hip_ok(hipMemset(qi->d_needed, 0, 2 * nb * 4), "hipMemset(needed)");
    if (ok && n_blocks)
        ok = hip_ok(hipMemcpy(qi->d_blocks, blocks, n_blocks * sizeof(dint_block_ref), hipMemcpyHostToDevice), "hipMemcpy(blocks)") &&
             hip_ok(hipMemcpy(qi->d_block_max, maxs.data(), n_blocks * 4, hipMemcpyHostToDevice), "hipMemcpy(block_max)");
    if (!ok) {
        dint_query_index_destroy(qi);
        return DINT_ERR_HIP;
    }
    *out = qi;
    return DINT_OK;
}

// The docs launch of `n_pages` prepared pages (units, spans, bases, left-as-gaps flags in the handle's workspaces), 256
// slots per page
static decode_request pages_request(dint_query_index* qi, size_t n_pages, uint32_t* d_docs, hipStream_t s) {
    decode_request r;
    r.dict = qi->docs, r.enc = qi->d_index, r.enc_bytes = qi->index_bytes, r.units = qi->units.p, r.n_units = n_pages;
    r.out = d_docs, r.out_capacity = size_t(n_pages) * kPageSlots, r.stream = s;
    r.only_full = 1, r.spans = qi->spans.p, r.unit_base = qi->bases.p, r.gaps_left = qi->gaps_left.p;
    return r;
}

// The pages of `sub` decoded, 256 slots per page, no sync: docs parts -> docIDs in d_docs (formed in the decode
// kernels' expansion, like dint_decode_block_table) and, with a freqs dictionary, freqs parts -> d_freqs.
static int decode_pages(dint_query_index* qi, size_t n_pages, uint32_t* d_docs, const dint_dict* freqs_dict, uint32_t* d_freqs,
                        hipStream_t s) {
    if (!qi->units.ensure(n_pages) || !qi->spans.ensure(n_pages) || !qi->bases.ensure(n_pages) || !qi->ends.ensure(n_pages) ||
        !qi->gaps_left.ensure(n_pages) || !qi->tails.ensure(n_pages + 1))
        return DINT_ERR_HIP;
    const uint32_t tb = 256;
    const uint32_t grid = uint32_t((n_pages + tb - 1) / tb);
    const uint64_t cap = uint64_t(n_pages) * kPageSlots;
    HIP_TRY(hipMemsetAsync(qi->gaps_left.p, 0, n_pages, s));
    HIP_TRY(hipMemsetAsync(qi->tails.p + n_pages, 0, 4, s));
    hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, qi->sub.p, static_cast<const uint64_t*>(nullptr),
                       uint64_t(n_pages), uint64_t(qi->index_bytes), qi->units.p, qi->spans.p, qi->bases.p);
    hipLaunchKernelGGL(collect_tails_kernel, dim3(grid), dim3(tb), 0, s, qi->sub.p, uint64_t(n_pages), qi->tails.p,
                       qi->tails.p + n_pages);
    decode_request docs = pages_request(qi, n_pages, d_docs, s);
    docs.end_off = qi->ends.p;
    int st = launch_decode(docs);
    if (st != DINT_OK) return st;
    if (freqs_dict) {  // freqs parts of the full blocks: from where their docs parts ended
        hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, qi->sub.p, qi->ends.p, uint64_t(n_pages),
                           uint64_t(qi->index_bytes), qi->units.p, qi->spans.p, static_cast<uint32_t*>(nullptr));
        decode_request freqs = pages_request(qi, n_pages, d_freqs, s);
        freqs.dict = freqs_dict, freqs.plus_one = 1, freqs.unit_base = nullptr, freqs.gaps_left = nullptr;
        st = launch_decode(freqs);
        if (st != DINT_OK) return st;
    }
    // (the grid is sized for "every page is a short block"; the waves past the list's end leave at once)
    hipLaunchKernelGGL(interpolative_tails_kernel, dim3(uint32_t((n_pages + kTailLanes - 1) / kTailLanes)), dim3(64), kTailLdsBytes, s,
                       qi->d_index, uint64_t(qi->index_bytes), qi->sub.p, static_cast<const uint64_t*>(nullptr), qi->tails.p,
                       qi->tails.p + n_pages, d_docs, cap, static_cast<uint64_t*>(nullptr), 0u, 1u, freqs_dict ? d_freqs : nullptr);
    hipLaunchKernelGGL(finalize_flagged_kernel, dim3(uint32_t((n_pages + 63) / 64)), dim3(64), 0, s, qi->sub.p, uint64_t(n_pages), d_docs,
                       cap, qi->gaps_left.p);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}

// Control words of one page decode (a call has one set for the candidates and one per round, cleared together):
// [0] blocks the round touched, [1] short pages, [kCtrlQueueAt ...) the decode kernel's queue counters.
constexpr size_t kCtrlQueueAt = 32;
constexpr size_t kCtrlWords = kCtrlQueueAt + (kQueueShards + 1) * kQueueStride;  // (the query kernels draw no chunk tickets: no chunk counters)

// A round's pages are decoded by decode_pages_lean (one launch) below this many pages, else by decode_pages_counted's
// three launches. Measured on the 1e8-posting index, in one process: the one-launch form wins at every size — a
// single query 95 -> 53 us, the reference's query log as one batch 2.16 -> 1.53 us per query, the longest lists
// 5.6 -> 5.0 — so it is the default; the variable keeps the other form testable (tests/test_gpu_queries.py).
static size_t lean_pages() {
    const long long v = opt(DINT_OPT_QUERY_LEAN_PAGES);
    return v < 0 ? ~size_t(0) : size_t(v);
}

// (one workgroup walks all the candidates: past a few pages the probe and search launches, a thread per candidate, win)
static size_t tail_pages() { return size_t(opt(DINT_OPT_QUERY_TAIL_PAGES)); }
// (a query of at most this many candidate pages runs as ONE launch of one workgroup: query_fused_body)
static size_t fused_pages() { return size_t(opt(DINT_OPT_QUERY_FUSED_PAGES)); }

// The one error path of the query calls once something may be running on the stream: wait for it, then the status.
static int stream_failed(hipStream_t s, int st) {
    (void)hipStreamSynchronize(s);
    return st;
}

// The blocks ids[0 .. *count) (count null: ids[0 .. n)) gathered and decoded by decode_pages, launches sized for n, as
// pages [at_page, at_page + n) of qi->probe and, with a freqs dictionary, of qi->fprobe.
static int gather_decode_pages(dint_query_index* qi, const uint32_t* d_ids, const uint32_t* d_count, size_t n, uint64_t at_page,
                               const dint_dict* freqs_dict, hipStream_t s) {
    const uint32_t tb = 256;
    hipLaunchKernelGGL(gather_pages_kernel, dim3(uint32_t((n + tb - 1) / tb)), dim3(tb), 0, s, qi->d_blocks, d_ids, uint64_t(n), qi->sub.p,
                       d_count);
    return decode_pages(qi, n, qi->probe.p + at_page * kPageSlots, freqs_dict, freqs_dict ? qi->fprobe.p + at_page * kPageSlots : nullptr, s);
}

// Pages -> docIDs in ONE launch: decode_*_query_kernel looks the blocks up itself, sums what it has to leave as gaps and
// runs the short blocks' interpolative code in place — no prepare, no schedule, no fix-up launch (for a single query
// the launches are what it waits for; in a batch the short blocks' bit-serial decoder, a launch of its own in the
// three-launch form, runs beside the full blocks instead of behind them). The arguments are decode_pages_counted's;
// `tail`: the round's tail, run by the same launch (round_tail).
static int decode_pages_lean(dint_query_index* qi, const uint32_t* d_ids, const uint32_t* d_count, size_t bound, uint32_t* d_docs,
                             uint32_t* ctrl, uint32_t retire, hipStream_t s, const query_pages* search, const round_tail* tail = nullptr) {
    if (!qi->gaps_left.ensure(bound)) return DINT_ERR_HIP;
    decode_args a = query_decode_args(qi);
    a.n_units = bound;
    a.out = d_docs;
    a.out_capacity = uint64_t(bound) * kPageSlots;
    a.gaps_left = qi->gaps_left.p;
    const uint32_t grid = decode_grid(qi->docs, bound);
    bind_counters(a, ctrl + kCtrlQueueAt, grid);
    query_pages qp{};
    if (search) qp = *search;  // (the first round's search, for the candidate pages)
    qp.blocks = qi->d_blocks;
    qp.ids = d_ids;
    qp.count = d_count;
    qp.bound = bound;
    qp.retire = retire;
    round_tail rt{};
    if (tail) rt = *tail;
    return query_decode_launch(qi, a, grid, s, decode_single_query_kernel, decode_multi_query_kernel, qp, rt);
}

// Pages -> docIDs, three launches on the stream: the pages are the blocks ids[0 .. *count) (count null: ids[0 .. bound)),
// `bound` >= their number is what the launches are sized for. `ctrl`: this decode's (cleared) control words.
// retire: the slots past each page's last posting are marked dead (candidate pages).
// `search` (candidate pages): what the first round's search needs; *searched says whether it was done along the way.
static int decode_pages_counted(dint_query_index* qi, const uint32_t* d_ids, const uint32_t* d_count, size_t bound, uint32_t* d_docs,
                                uint32_t* ctrl, uint32_t retire, hipStream_t s, const query_pages* search = nullptr,
                                bool* searched = nullptr) {
    if (searched) *searched = false;
    if (bound < lean_pages() && qi->index_bytes >= 8) {
        if (searched) *searched = search != nullptr;
        return decode_pages_lean(qi, d_ids, d_count, bound, d_docs, ctrl, retire, s, search);
    }
    if (!qi->sub.ensure(bound) || !qi->units.ensure(bound) || !qi->spans.ensure(bound) || !qi->bases.ensure(bound) ||
        !qi->ends.ensure(bound) || !qi->gaps_left.ensure(bound) || !qi->tails.ensure(bound + 1))
        return DINT_ERR_HIP;
    const uint32_t tb = 256;
    const uint64_t cap = uint64_t(bound) * kPageSlots;
    uint32_t* const d_n_tails = ctrl + 1;
    hipLaunchKernelGGL(prepare_pages_kernel, dim3(uint32_t((bound + tb - 1) / tb)), dim3(tb), 0, s, qi->d_blocks, uint64_t(qi->n_blocks),
                       uint64_t(qi->index_bytes), d_ids, d_count, uint64_t(bound), qi->sub.p, qi->units.p, qi->spans.p, qi->bases.p,
                       qi->gaps_left.p, qi->tails.p, d_n_tails);
    decode_request docs = pages_request(qi, bound, d_docs, s);
    docs.schedule_from = 2048, docs.zeroed_queue = ctrl + kCtrlQueueAt;
    int st = launch_decode(docs);
    if (st != DINT_OK) return st;
    // (the grid is sized for "every page is a short block": the waves with nothing to do leave at once)
    hipLaunchKernelGGL(fix_pages_kernel, dim3(uint32_t((bound + kTailLanes - 1) / kTailLanes)), dim3(64), kTailLdsBytes, s, qi->d_index,
                       uint64_t(qi->index_bytes), qi->sub.p, uint64_t(bound), qi->tails.p, d_n_tails, d_docs, cap, qi->gaps_left.p, retire);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}
