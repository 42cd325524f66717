// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": conjunctive queries (queries.hpp:34-84).
// ---- conjunctive queries ------------------------------------------------------------------------

void dint_query_index_destroy(dint_query_index* qi) {
    if (!qi) return;
    (void)hipSetDevice(qi->device);  // (the workspaces are freed by delete, on this device; qi->docs may be gone already)
    for (void* p : {static_cast<void*>(qi->d_blocks), static_cast<void*>(qi->d_block_max), static_cast<void*>(qi->d_needed),
                    static_cast<void*>(qi->d_rank), static_cast<void*>(qi->d_touched)})
        if (p) (void)hipFree(p);
    if (qi->h_stage) (void)hipHostFree(qi->h_stage);
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
    std::vector<uint32_t> maxs(n_blocks);
    uint32_t prev_list = 0;
    for (size_t b = 0; b != n_blocks; ++b) {
        const uint32_t l = blocks[b].list;
        // lists in order, each list's blocks contiguous; docID 0xFFFFFFFF is kDeadCandidate, no docID (num_docs <= 2^32 - 1)
        if (l >= n_lists || l < prev_list || blocks[b].n == 0 || blocks[b].n > 256 || blocks[b].in_off > index_bytes ||
            blocks[b].max == 0xFFFFFFFFu) {
            delete qi;
            return DINT_ERR_FORMAT;
        }
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
    int st = launch_decode(qi->docs, qi->d_index, qi->index_bytes, qi->units.p, n_pages, d_docs, cap, qi->ends.p, s, 1, qi->spans.p, 0,
                           qi->bases.p, qi->gaps_left.p);
    if (st != DINT_OK) return st;
    if (freqs_dict) {  // freqs parts of the full blocks: from where their docs parts ended
        hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, qi->sub.p, qi->ends.p, uint64_t(n_pages),
                           uint64_t(qi->index_bytes), qi->units.p, qi->spans.p, static_cast<uint32_t*>(nullptr));
        st = launch_decode(freqs_dict, qi->d_index, qi->index_bytes, qi->units.p, n_pages, d_freqs, cap, nullptr, s, 1, qi->spans.p, 1);
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
static int decode_pages_lean(dint_query_index* qi, const uint32_t* d_ids, const uint32_t* d_count, size_t bound, uint32_t* d_docs,
                             uint32_t* ctrl, uint32_t retire, hipStream_t s, const query_pages* search,
                             const round_tail* tail = nullptr);

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
    int st = launch_decode(qi->docs, qi->d_index, qi->index_bytes, qi->units.p, bound, d_docs, cap, nullptr, s, 1, qi->spans.p, 0,
                           qi->bases.p, qi->gaps_left.p, nullptr, 2048, ctrl + kCtrlQueueAt);
    if (st != DINT_OK) return st;
    // (the grid is sized for "every page is a short block": the waves with nothing to do leave at once)
    hipLaunchKernelGGL(fix_pages_kernel, dim3(uint32_t((bound + kTailLanes - 1) / kTailLanes)), dim3(64), kTailLdsBytes, s, qi->d_index,
                       uint64_t(qi->index_bytes), qi->sub.p, uint64_t(bound), qi->tails.p, d_n_tails, d_docs, cap, qi->gaps_left.p, retire);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}

// The same in ONE launch: decode_*_query_kernel looks the blocks up itself, sums what it has to leave as gaps and
// runs the short blocks' interpolative code in place — no prepare, no schedule, no fix-up launch (for a single query
// the launches are what it waits for; in a batch the short blocks' bit-serial decoder, a launch of its own in the
// three-launch form, runs beside the full blocks instead of behind them).
static int decode_pages_lean(dint_query_index* qi, const uint32_t* d_ids, const uint32_t* d_count, size_t bound, uint32_t* d_docs,
                             uint32_t* ctrl, uint32_t retire, hipStream_t s, const query_pages* search, const round_tail* tail) {
    if (!qi->gaps_left.ensure(bound)) return DINT_ERR_HIP;
    const dint_dict* dd = qi->docs;
    decode_args a{};
    a.dict = dd->view;
    a.enc = qi->d_index;
    a.enc_bytes = qi->index_bytes;
    a.n_units = bound;
    a.out = d_docs;
    a.out_capacity = uint64_t(bound) * kPageSlots;
    a.gaps_left = qi->gaps_left.p;
    const uint64_t blocks_needed = (uint64_t(bound) + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint32_t grid = uint32_t(std::min<uint64_t>(blocks_needed, std::max<uint32_t>(1, dd->compute_units) * kBlocksPerCU));
    const size_t lds_bytes = (size_t(dd->view.hot_words) + kClassTableWords + kWavesPerBlock * kScratchWords) * 4;
    a.queue = ctrl + kCtrlQueueAt;
    a.chunk_queue = a.queue + kQueueShards * kQueueStride;
    a.clock = reinterpret_cast<uint64_t*>(a.chunk_queue + kClockWordAt);
    a.n_shards = std::min<uint32_t>(kQueueShards, grid);
    query_pages qp{};
    if (search) qp = *search;  // (the first round's search, for the candidate pages)
    qp.blocks = qi->d_blocks;
    qp.ids = d_ids;
    qp.count = d_count;
    qp.bound = bound;
    qp.retire = retire;
    round_tail rt{};
    if (tail) rt = *tail;
    if (dd->kind == DINT_DICT_MULTI_PACKED)
        hipLaunchKernelGGL(decode_multi_query_kernel, dim3(grid), dim3(kBlockThreads), lds_bytes, s, a, qp, rt);
    else
        hipLaunchKernelGGL(decode_single_query_kernel, dim3(grid), dim3(kBlockThreads), lds_bytes, s, a, qp, rt);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}

// Per query: its distinct terms (queries.hpp:28-31, 49-52, 92) by list length, ascending (AND: the rarest list first) or
// descending (OR: the longest list probes nothing), equal lengths by term id, and (with_qf) each term's multiplicity
// beside it (query_freqs, queries.hpp:135-148). One flat copy of the call's terms, every query's part planned in place
// (a vector per query was an allocation per query: a third of a batch call's host time).
struct query_plan {
    const uint64_t* offsets = nullptr;
    uint64_t first = 0;
    std::vector<uint32_t> terms, qf;
    std::vector<uint32_t> len;  // planned terms of query q; 0: none, or nothing to launch (one list, counted on the host)
    const uint32_t* of(size_t q) const { return terms.data() + (offsets[q] - first); }
    const uint32_t* qf_of(size_t q) const { return qf.data() + (offsets[q] - first); }
};

// Checks the offsets and every term before anything is written (DINT_ERR_ARG), then plans the queries: counts[q] and
// freq_sums[q] (if given) <- 0, and without freqs a query of one list is answered here, counts[q] <- the list's length.
static int plan_queries(const dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                        bool longest_first, bool with_qf, bool with_freqs, uint64_t* counts, uint64_t* freq_sums, query_plan& plan) {
    if (query_offsets[0] != 0 && !terms) return DINT_ERR_ARG;
    for (size_t q = 0; q != n_queries; ++q)
        if (query_offsets[q + 1] < query_offsets[q] || (query_offsets[q + 1] > query_offsets[q] && !terms)) return DINT_ERR_ARG;
    const uint64_t t_first = query_offsets[0], t_all = query_offsets[n_queries] - t_first;
    for (uint64_t i = 0; i != t_all; ++i)
        if (terms[t_first + i] >= qi->list_len.size()) return DINT_ERR_ARG;
    plan.offsets = query_offsets;
    plan.first = t_first;
    plan.terms.assign(terms ? terms + t_first : nullptr, terms ? terms + t_first + t_all : nullptr);
    plan.qf.assign(with_qf ? t_all : 0, 0u);
    plan.len.assign(n_queries, 0u);
    const uint32_t* const len = qi->list_len.data();
    for (size_t q = 0; q != n_queries; ++q) {
        uint32_t* const t = plan.terms.data() + (query_offsets[q] - t_first);
        uint32_t* const qf = with_qf ? plan.qf.data() + (query_offsets[q] - t_first) : nullptr;
        // (equal terms end up side by side in this order: one pass drops them and counts them)
        std::sort(t, t + (query_offsets[q + 1] - query_offsets[q]), [&](uint32_t a, uint32_t b) {
            return len[a] != len[b] ? (longest_first ? len[a] > len[b] : len[a] < len[b]) : a < b;
        });
        uint32_t n = 0;
        for (uint64_t i = 0; i != query_offsets[q + 1] - query_offsets[q]; ++i) {
            if (n != 0 && t[i] == t[n - 1]) {
                if (qf) qf[n - 1] += 1;
                continue;
            }
            if (qf) qf[n] = 1;
            t[n++] = t[i];
        }
        counts[q] = 0;
        if (freq_sums) freq_sums[q] = 0;
        if (n == 1 && !with_freqs)  // one list: every posting is a result (and_query<false> would walk it and count)
            counts[q] = len[t[0]];
        else
            plan.len[q] = n;
    }
    return DINT_OK;
}

// dint_ranked_and_queries (hip_api_ranked_query.inc), dint_ranked_or_queries: what the freqs pass scores with, and where
// the selection goes
struct ranked_args {
    const float* norm_lens;    // device, the wand handle's
    uint32_t k;
    unsigned long long* keys;  // host, n_queries * k: the best keys of every query (ranked_topk)
    uint64_t num_docs;         // the wand handle's
};
// bm25::query_term_weight (bm25.hpp), binary32 in its source order: qf = the term's multiplicity, df = its list's length
static float bm25_query_term_weight(uint32_t qf, uint64_t df, uint64_t num_docs) {
    const float f = float(qf);
    const float fdf = float(df);
    const float idf = std::log((float(num_docs) - fdf + 0.5f) / (fdf + 0.5f));
    const float epsilon_score = 1.0E-6f;
    return f * std::max(epsilon_score, idf) * (1.0f + kBm25K1);
}
static int ranked_topk(dint_query_index* qi, const ranked_args& rk, const std::vector<uint32_t>& page_query, size_t n_queries,
                       hipStream_t s);

static int and_queries_impl(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                            size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks, void* stream, bool may_split = true,
                            const ranked_args* rk = nullptr);

// the *_queries_freqs entries: a freqs dictionary of the index's device and kind, and somewhere for the sums
static bool freqs_args_ok(const dint_query_index* qi, const dint_dict* freqs_dict, const uint64_t* freq_sums) {
    return freqs_dict && freq_sums && (!qi || (freqs_dict->device == qi->docs->device && freqs_dict->kind == qi->docs->kind));
}

int dint_and_queries(dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                     uint64_t* counts, void* stream) {
    return and_queries_impl(qi, nullptr, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream);
}

int dint_and_queries_freqs(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                           size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks_decoded, void* stream) {
    if (!freqs_args_ok(qi, freqs_dict, freq_sums)) return DINT_ERR_ARG;
    return and_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums, freq_blocks_decoded, stream);
}

static int and_queries_impl(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                            size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks, void* stream, bool may_split,
                            const ranked_args* rk) {
    if (!qi || (n_queries && (!query_offsets || !counts))) return DINT_ERR_ARG;
    if (freq_blocks) *freq_blocks = 0;
    if (n_queries == 0) return DINT_OK;
    if (n_queries >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    query_plan plan;
    const int planned = plan_queries(qi, terms, query_offsets, n_queries, false, rk != nullptr, freqs_dict != nullptr, counts, freq_sums, plan);
    if (planned != DINT_OK) return planned;
    size_t rounds = 0;
    std::vector<uint32_t> h_page_block, h_page_query;
    h_page_block.reserve(n_queries + 64);
    h_page_query.reserve(n_queries + 64);
    for (size_t q = 0; q != n_queries; ++q) {
        if (plan.len[q] == 0) continue;
        rounds = std::max<size_t>(rounds, plan.len[q] - 1);
        const uint32_t rarest = plan.of(q)[0];
        for (uint32_t b = qi->list_first[rarest]; b != qi->list_first[rarest + 1]; ++b) {
            h_page_block.push_back(b);
            h_page_query.push_back(uint32_t(q));
        }
    }
    const size_t n_pages = h_page_block.size();
    if (n_pages == 0) return DINT_OK;
    // A MIXED call — queries of a few candidate pages among queries of hundreds: the small ones go through the
    // workgroup-per-query launch (below), the others through the round-per-launch form, as two calls of this function over the
    // sorted plans (a single large query no longer takes a log of small ones onto the slow form with it).
    if (may_split && !freqs_dict && n_queries >= 3 && opt(DINT_OPT_QUERY_BATCH_FUSED) != 0) {
        size_t n_small = 0, n_large = 0;
        for (size_t q = 0; q != n_queries; ++q)
            if (plan.len[q] != 0) {
                const uint32_t rarest = plan.of(q)[0];
                (qi->list_first[rarest + 1] - qi->list_first[rarest] <= kBatchPages ? n_small : n_large) += 1;
            }
        if (n_small >= 2 && n_large != 0) {
            for (int part = 0; part != 2; ++part) {  // 0: the small queries, 1: the others
                std::vector<uint32_t> sub_terms, sub_q;
                std::vector<uint64_t> sub_offs(1, 0);
                for (size_t q = 0; q != n_queries; ++q)
                    if (plan.len[q] != 0) {
                        const uint32_t rarest = plan.of(q)[0];
                        const bool is_small = qi->list_first[rarest + 1] - qi->list_first[rarest] <= kBatchPages;
                        if (is_small != (part == 0)) continue;
                        sub_terms.insert(sub_terms.end(), plan.of(q), plan.of(q) + plan.len[q]);
                        sub_offs.push_back(sub_terms.size());
                        sub_q.push_back(uint32_t(q));
                    }
                std::vector<uint64_t> sub_counts(sub_q.size(), 0);
                const int st = and_queries_impl(qi, nullptr, sub_terms.data(), sub_offs.data(), sub_q.size(), sub_counts.data(), nullptr, nullptr, stream, false);
                if (st != DINT_OK) return st;
                for (size_t k = 0; k != sub_q.size(); ++k) counts[sub_q[k]] = sub_counts[k];
            }
            return DINT_OK;
        }
    }
    const uint64_t n_slots = uint64_t(n_pages) * kPageSlots;
    std::vector<uint32_t> h_first(std::max<size_t>(1, rounds * n_queries), 0), h_blocks(std::max<size_t>(1, rounds * n_queries), 0);
    for (size_t q = 0; q != n_queries; ++q)
        for (size_t j = 1; j < plan.len[q]; ++j) {
            const uint32_t l = plan.of(q)[j];
            h_first[(j - 1) * n_queries + q] = qi->list_first[l];
            h_blocks[(j - 1) * n_queries + q] = qi->list_first[l + 1] - qi->list_first[l];
        }

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // ---- a call of SMALL queries (a few candidate pages each — the reference's log): a workgroup per query, ONE launch
    // (query_batch_body; DINT_OPT_QUERY_BATCH_FUSED = 0: the round-per-launch batch form below, as until late in round 5) ----
    {
        bool small = !freqs_dict && n_queries >= 2 && rounds != 0 && qi->index_bytes >= 8 && opt(DINT_OPT_QUERY_BATCH_FUSED) != 0 && n_pages < 0xFFFFFFFFull / kPageSlots;
        std::vector<uint32_t> rec;   // per active query: {query, first page, pages, steps} then {probe page, control word}
        uint64_t probe_pages = 0, ctrl_at = 0;
        bool any_full = false;
        if (small) {
            rec.reserve(6 * n_queries);
            size_t page = 0;
            for (size_t q = 0; q != n_queries && small; ++q) {
                if (plan.len[q] == 0) continue;
                const uint32_t rarest = plan.of(q)[0];
                const uint32_t pages_q = qi->list_first[rarest + 1] - qi->list_first[rarest];
                small = pages_q <= kBatchPages && plan.len[q] >= 2;
                uint64_t most = 0;
                for (uint32_t j = 1; j != plan.len[q]; ++j) most = std::max<uint64_t>(most, h_blocks[(j - 1) * n_queries + q]);
                for (uint32_t j = 0; j != plan.len[q]; ++j) any_full = any_full || qi->list_len[plan.of(q)[j]] >= kBlock;
                const uint64_t stretch = std::min<uint64_t>(most, uint64_t(pages_q) * kPageSlots);
                rec.insert(rec.end(), {uint32_t(q), uint32_t(page), pages_q, plan.len[q], uint32_t(probe_pages), uint32_t(ctrl_at)});
                page += pages_q;
                probe_pages += stretch;
                ctrl_at += uint64_t(plan.len[q]) * kBatchCtrlWords;
                small = small && probe_pages < (1ull << 22) && ctrl_at < (1ull << 30);
            }
        }
        const size_t n_active = rec.size() / 6;
        if (small && n_active != 0) {
            const dint_dict* dd = qi->docs;
            const uint32_t grid = uint32_t(std::min<size_t>(n_active, std::max<uint32_t>(1, dd->compute_units) * kBlocksPerCU));
            // (per workgroup two hashed claim tables and two touched lists: 160 KB, whatever the index's size)
            const size_t slot_words = size_t(grid) * 2 * kBatchClaimSlots, touched_words = size_t(grid) * 2 * kBatchTouched;
            const size_t tab_words = (2 * n_pages + h_first.size() + h_blocks.size() + 3) / 4 * 4;
            const size_t cnt_words = (2 * n_queries + 3) / 4 * 4;  // the result counters (u64 each): zeros, copied in with the tables
            const size_t up = tab_words + cnt_words + 6 * n_active;
            const size_t stage_bytes = std::max(up * 4, n_queries * sizeof(unsigned long long));
            HIP_TRY(qi->stage(stage_bytes));
            if (qi->d_stage != nullptr) {
                if (!qi->inputs.ensure(up + 4) || !qi->cand.ensure(n_slots) || !qi->target.ensure(n_slots) ||
                    !qi->probe.ensure(std::max<uint64_t>(1, probe_pages) * kPageSlots) || !qi->gaps_left.ensure(n_pages + probe_pages + 1) ||
                    !qi->batch_ctrl.ensure(std::max<uint64_t>(1, ctrl_at)) || !qi->slot_rank.ensure(slot_words) || !qi->slot_touched.ensure(touched_words))
                    return DINT_ERR_HIP;
                if (qi->slot_needed.cap < slot_words) qi->slot_needed_clean = 0;  // (ensure() below hands out a new, unwritten buffer)
                if (!qi->slot_needed.ensure(slot_words)) return DINT_ERR_HIP;
                if (qi->slot_needed_clean < qi->slot_needed.cap || qi->slots_dirty) {
                    HIP_TRY(hipMemsetAsync(qi->slot_needed.p, 0, qi->slot_needed.cap * 4, s));
                    qi->slot_needed_clean = qi->slot_needed.cap;
                    qi->slots_dirty = false;
                }
                uint32_t* const h = static_cast<uint32_t*>(qi->h_stage);
                std::memcpy(h, h_page_block.data(), n_pages * 4);
                std::memcpy(h + n_pages, h_page_query.data(), n_pages * 4);
                std::memcpy(h + 2 * n_pages, h_first.data(), h_first.size() * 4);
                std::memcpy(h + 2 * n_pages + h_first.size(), h_blocks.data(), h_blocks.size() * 4);
                std::memset(h + tab_words, 0, cnt_words * 4);
                uint32_t* const hq = h + tab_words + cnt_words;  // {q, page, pages, steps} x n, then {probe page, control word} x n
                for (size_t k = 0; k != n_active; ++k) {
                    std::memcpy(hq + 4 * k, &rec[6 * k], 16);
                    std::memcpy(hq + 4 * n_active + 2 * k, &rec[6 * k + 4], 8);
                }
                HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, up * 4, hipMemcpyHostToDevice, s));
                fused_batch b{};
                b.page_block = qi->inputs.p;
                b.page_query = b.page_block + n_pages;
                b.term_first = b.page_query + n_pages;
                b.term_blocks = b.term_first + h_first.size();
                b.n_queries = uint32_t(n_queries);
                b.n_active = uint32_t(n_active);
                b.block_max = qi->d_block_max;
                b.blocks = qi->d_blocks;
                b.qrec = reinterpret_cast<const u32x4*>(qi->inputs.p + tab_words + cnt_words);
                b.qrec2 = reinterpret_cast<const u32x2*>(qi->inputs.p + tab_words + cnt_words + 4 * n_active);
                b.cand = qi->cand.p;
                b.target = qi->target.p;
                b.probe = qi->probe.p;
                b.gaps_left = qi->gaps_left.p;
                b.probe_flags_at = n_pages;
                b.ctrl = qi->batch_ctrl.p;
                b.needed = qi->slot_needed.p;
                b.rank = qi->slot_rank.p;
                b.touched = qi->slot_touched.p;
                b.counts = reinterpret_cast<unsigned long long*>(qi->inputs.p + tab_words);
                b.host_counts = static_cast<unsigned long long*>(qi->d_stage);
                decode_args a{};
                a.dict = dd->view;
                a.enc = qi->d_index;
                a.enc_bytes = qi->index_bytes;
                if (!any_full) a.dict.hot_words = 0;  // (short blocks only: nothing reads the dictionary's image)
                const size_t lds_bytes = (size_t(a.dict.hot_words) + kClassTableWords + kWavesPerBlock * kScratchWords) * 4;
                qi->slots_dirty = true;  // until the call has run to its end
                if (dd->kind == DINT_DICT_MULTI_PACKED)
                    hipLaunchKernelGGL(decode_multi_query_batch_kernel, dim3(grid), dim3(kBlockThreads), lds_bytes, s, a, b);
                else
                    hipLaunchKernelGGL(decode_single_query_batch_kernel, dim3(grid), dim3(kBlockThreads), lds_bytes, s, a, b);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipStreamSynchronize(s));
                qi->slots_dirty = false;
                const unsigned long long* const h_counts = static_cast<const unsigned long long*>(qi->h_stage);
                for (size_t q = 0; q != n_queries; ++q)
                    if (plan.len[q] != 0) counts[q] = h_counts[q];
                return DINT_OK;
            }
        }
    }
    // inputs: {page -> block, page -> query, per round and query: first block and block count of the round's list},
    // and behind them — zeros, copied in with them: one copy instead of a copy and a clear — every counter the
    // call's launches count in, and the result counters (u64 each)
    const size_t in_words = (2 * n_pages + h_first.size() + h_blocks.size() + 31) / 32 * 32;
    const size_t ctrl_words = ((rounds + 1) * kCtrlWords + 2 * n_queries + 1) / 2 * 2;
    const size_t step_words = (rounds + 1) * ((sizeof(fused_step) + 7) / 8 * 2);  // (the one-launch form's steps, 8-byte aligned)
    const size_t up_words = in_words + ctrl_words + step_words;
    const size_t stage_bytes = std::max(up_words * 4, n_queries * sizeof(unsigned long long));
    HIP_TRY(qi->stage(stage_bytes));  // (d_stage: the last probe writes the results there)
    if (!qi->inputs.ensure(up_words + 4) || !qi->cand.ensure(n_slots) || !qi->target.ensure(n_slots)) return DINT_ERR_HIP;
    {
        uint32_t* h = static_cast<uint32_t*>(qi->h_stage);
        std::memcpy(h, h_page_block.data(), n_pages * 4);
        std::memcpy(h + n_pages, h_page_query.data(), n_pages * 4);
        std::memcpy(h + 2 * n_pages, h_first.data(), h_first.size() * 4);
        std::memcpy(h + 2 * n_pages + h_first.size(), h_blocks.data(), h_blocks.size() * 4);
        std::memset(h + in_words, 0, ctrl_words * 4);
    }
    uint32_t* const d_page_block = qi->inputs.p;
    uint32_t* const d_page_query = d_page_block + n_pages;
    uint32_t* const d_term_first = d_page_query + n_pages;
    uint32_t* const d_term_blocks = d_term_first + h_first.size();
    uint32_t* const d_ctrl = qi->inputs.p + in_words;
    unsigned long long* const d_counts = reinterpret_cast<unsigned long long*>(d_ctrl + (rounds + 1) * kCtrlWords);
    // Round r's tail (and_round_tail_kernel, or a one-launch form's step): its probe, the release of its claims, and then
    // either the next round's block-max search — the two rounds' claim sets alternate — or (last) the count of the
    // survivors, also written to host_counts unless that is null. Its page decode counts in ctrl = d_ctrl + (r + 1) * kCtrlWords.
    const size_t nb = std::max<size_t>(1, qi->n_blocks);
    auto tail_of_round = [&](size_t r, bool last, unsigned long long* host_counts) {
        const size_t set = r & 1, next_set = set ^ 1;
        uint32_t* const ctrl = d_ctrl + (r + 1) * kCtrlWords;
        round_tail t{};
        t.done = ctrl + 2;  // (not counted in: non-null says "this step has a tail")
        t.cand = qi->cand.p;
        t.n_slots = n_slots;
        t.page_query = d_page_query;
        t.blocks = qi->d_blocks;
        t.target = qi->target.p;
        t.term_blocks = d_term_blocks + r * n_queries;
        t.rank = qi->d_rank + set * nb;
        t.probe = qi->probe.p;
        t.touched = qi->d_touched + set * nb;
        t.n_touched = ctrl;
        t.needed = qi->d_needed + set * nb;
        if (!last) {
            t.next_first = d_term_first + (r + 1) * n_queries;
            t.next_blocks = d_term_blocks + (r + 1) * n_queries;
            t.block_max = qi->d_block_max;
            t.next_needed = qi->d_needed + next_set * nb;
            t.next_rank = qi->d_rank + next_set * nb;
            t.next_touched = qi->d_touched + next_set * nb;
            t.next_n_touched = d_ctrl + (r + 2) * kCtrlWords;
        } else {
            t.counts = d_counts;
            t.host_counts = host_counts;
            t.n_queries = uint32_t(n_queries);
        }
        return t;
    };
    // ---- what the host knows of the rounds before anything runs: a bound of the pages each decodes ------------------
    uint64_t round0_blocks = 0;
    if (rounds)
        for (size_t q = 0; q != n_queries; ++q) round0_blocks += h_blocks[q];
    std::vector<size_t> round_bound(rounds, 0);
    bool small_rounds = rounds != 0 && round0_blocks != 0 && n_pages < lean_pages() && qi->index_bytes >= 8;
    for (size_t r = 0; r != rounds; ++r) {
        uint64_t list_blocks = 0;
        for (size_t q = 0; q != n_queries; ++q) list_blocks += h_blocks[r * n_queries + q];
        round_bound[r] = size_t(std::min<uint64_t>(n_slots, list_blocks));
        small_rounds = small_rounds && list_blocks != 0 && round_bound[r] < lean_pages();
    }
    // A query of a page or two of candidates: the whole chain — candidates, then every round's pages and tail — in ONE
    // launch of one workgroup (query_fused_body; DINT_QUERY_FUSED_PAGES: at most that many candidate pages, 0: never).
    const bool fused_ok = small_rounds && n_pages <= tail_pages() && n_pages <= fused_pages();
    fused_step* const d_steps = reinterpret_cast<fused_step*>(qi->inputs.p + in_words + ctrl_words);
    if (fused_ok) {
        size_t max_pages = n_pages;
        for (size_t r = 0; r != rounds; ++r) max_pages = std::max(max_pages, round_bound[r]);
        if (!qi->probe.ensure(uint64_t(max_pages) * kPageSlots) || !qi->gaps_left.ensure(max_pages)) return DINT_ERR_HIP;
        fused_step* const h_steps = reinterpret_cast<fused_step*>(static_cast<uint32_t*>(qi->h_stage) + in_words + ctrl_words);
        const bool to_host = !freqs_dict && qi->d_stage != nullptr;
        for (size_t k = 0; k != rounds + 1; ++k) {
            fused_step st{};
            st.gaps_left = qi->gaps_left.p;
            st.qp.blocks = qi->d_blocks;
            if (k == 0) {  // the candidate pages, the first round's search riding along (decode_pages_lean's candidate call)
                st.out = qi->cand.p;
                st.out_capacity = uint64_t(n_pages) * kPageSlots;
                st.qp.page_query = d_page_query;
                st.qp.term_first = d_term_first;
                st.qp.term_blocks = d_term_blocks;
                st.qp.block_max = qi->d_block_max;
                st.qp.target = qi->target.p;
                st.qp.needed = qi->d_needed;
                st.qp.rank = qi->d_rank;
                st.qp.touched = qi->d_touched;
                st.qp.n_touched = d_ctrl + kCtrlWords;
                st.qp.ids = d_page_block;
                st.qp.count = nullptr;
                st.qp.bound = n_pages;
                st.qp.retire = 1u;
            } else {  // round r: the touched pages, then the tail (the round-per-launch form's round_tail, below)
                const size_t r = k - 1;
                st.out = qi->probe.p;
                st.out_capacity = uint64_t(round_bound[r]) * kPageSlots;
                st.qp.ids = qi->d_touched + (r & 1) * nb;
                st.qp.count = d_ctrl + (r + 1) * kCtrlWords;
                st.qp.bound = round_bound[r];
                st.qp.retire = 0u;
                st.rt = tail_of_round(r, r + 1 == rounds, to_host ? static_cast<unsigned long long*>(qi->d_stage) : nullptr);
            }
            std::memcpy(h_steps + k, &st, sizeof st);
        }
    }
    // (the one-launch form's workgroup brings the inputs over itself — fused_inputs: no copy on the stream in front of it)
    const bool bring_inputs = fused_ok && qi->d_stage != nullptr && opt(DINT_OPT_QUERY_FUSED_COPY) != 0;
    if (!bring_inputs) HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, up_words * 4, hipMemcpyHostToDevice, s));

    const uint32_t tb = 256;
    const uint32_t slot_grid = uint32_t(n_pages);  // 256 slots per page = one workgroup
    if (qi->claims_dirty) {  // (a call that failed between a search and its release left claim flags behind)
        HIP_TRY(hipMemsetAsync(qi->d_needed, 0, 2 * std::max<size_t>(1, qi->n_blocks) * 4, s));
        qi->claims_dirty = false;
    }
    // candidates: the rarest list of every query
    query_pages search0{};
    search0.page_query = d_page_query;
    search0.term_first = d_term_first;
    search0.term_blocks = d_term_blocks;
    search0.block_max = qi->d_block_max;
    search0.target = qi->target.p;
    search0.needed = qi->d_needed;
    search0.rank = qi->d_rank;
    search0.touched = qi->d_touched;
    search0.n_touched = d_ctrl + kCtrlWords;
    bool searched0 = false;
    int st = DINT_OK;
    if (fused_ok) {
        const dint_dict* dd = qi->docs;
        decode_args a{};
        a.dict = dd->view;
        a.enc = qi->d_index;
        a.enc_bytes = qi->index_bytes;
        // lists of fewer than 256 postings are one interpolative block each and need no dictionary: a query of such lists
        // only (most of a query log's) runs without the 88 KB LDS image — nothing reads it
        bool any_full = false;
        for (size_t q = 0; q != n_queries; ++q)
            for (uint32_t j = 0; j != plan.len[q]; ++j) any_full = any_full || qi->list_len[plan.of(q)[j]] >= kBlock;
        if (!any_full) a.dict.hot_words = 0;
        const size_t lds_bytes = (size_t(a.dict.hot_words) + kClassTableWords + kWavesPerBlock * kScratchWords) * 4;
        fused_inputs bring{};
        if (bring_inputs) {
            bring.from = static_cast<const u32x4*>(qi->d_stage);
            bring.to = reinterpret_cast<u32x4*>(qi->inputs.p);
            bring.words = uint32_t((up_words + 3) / 4 * 4);  // (both buffers end beyond that)
        }
        if (dd->kind == DINT_DICT_MULTI_PACKED)
            hipLaunchKernelGGL(decode_multi_query_fused_kernel, dim3(1), dim3(kBlockThreads), lds_bytes, s, a, d_steps, uint32_t(rounds + 1), bring);
        else
            hipLaunchKernelGGL(decode_single_query_fused_kernel, dim3(1), dim3(kBlockThreads), lds_bytes, s, a, d_steps, uint32_t(rounds + 1), bring);
        HIP_TRY(hipGetLastError());
        searched0 = true;
    } else {
        st = decode_pages_counted(qi, d_page_block, nullptr, n_pages, qi->cand.p, d_ctrl, 1u, s, round0_blocks ? &search0 : nullptr, &searched0);
    }
    if (st != DINT_OK) {
        (void)hipStreamSynchronize(s);
        return st;
    }
    qi->claims_dirty = true;  // until the call has run to its end

    // A round: block-max search -> the touched blocks, without duplicates -> decoded -> every candidate probes its
    // block. How many blocks a round touches only the device knows; the host knows a bound (the live candidates at
    // most, and no more blocks than the round's lists have) and sizes the launches for that — nothing on the host
    // waits for a round: a call is one copy in, then per round search, page decode, probe. (Round 1 read the
    // count back every round and made fourteen API calls per round: a query at a time, the host's share was most of
    // the 200 us a query took.) Past kAsyncPages the count is read back after all — the probe buffer is sized for the
    // bound, a kilobyte a page. (Until late in round 5 the limit was 32768 pages: a launch sized for a bound far above the
    // truth cost more than the wait while every workgroup of it loaded the dictionary's image and swept the ticket
    // counters; now an idle workgroup leaves at once, and the heavy log's call without its three mid-call waits is
    // 3.55 against 3.68 us per query.)
    constexpr size_t kAsyncPages = size_t(1) << 20;
    // ... and the workspace a bound may claim on its own: a kilobyte a page, never shrunk (device_buffer). A bound that asks
    // for more than this AND more than the index already owns is read back instead (4 bytes, one wait) and the buffers are
    // sized for the truth; so is a bound whose allocation fails. Worst case kept by one dint_query_index for the probe pages
    // (and_queries_freqs: twice, docs and freqs): max(256 MiB, 1.5 x the largest exact count seen) — include/dint_hip.h.
    constexpr size_t kAsyncProbeWords = (size_t(256) << 20) / 4;
    auto sized_by_bound = [&](size_t bound, std::initializer_list<std::pair<device_buffer<uint32_t>*, size_t>> bufs) {
        if (bound > kAsyncPages) return false;
        for (auto const& b : bufs)
            if (b.second > kAsyncProbeWords && b.second > b.first->cap) return false;
        for (auto const& b : bufs)
            if (!b.first->ensure(b.second)) {
                (void)hipGetLastError();  // (out of memory for the bound: the exact count may still fit)
                return false;
            }
        return true;
    };
    size_t last_round = rounds;  // the last round that has anything to probe counts the survivors as well
    for (size_t r = 0; r != rounds; ++r)
        for (size_t q = 0; q != n_queries; ++q)
            if (h_blocks[r * n_queries + q]) {
                last_round = r;
                break;
            }
    bool counted = false;
    // the last probe hands the results over itself (a few pages: every workgroup of it passes through one counter)
    bool results_to_host = !freqs_dict && qi->d_stage != nullptr && n_pages <= 4096;
    // Few candidates, few pages in every round (a single query): one launch per round — round_tail.
    const bool tail_form = searched0 && small_rounds && n_pages <= tail_pages();
    if (fused_ok) {
        counted = true;  // (the launch above was the whole query)
        results_to_host = results_to_host && qi->d_stage != nullptr;
    }
    unsigned long long* const host_counts = results_to_host ? static_cast<unsigned long long*>(qi->d_stage) : nullptr;
    if (tail_form && !fused_ok) {
        for (size_t r = 0; r != rounds; ++r) {
            uint32_t* const ctrl = d_ctrl + (r + 1) * kCtrlWords;
            if (!qi->probe.ensure(uint64_t(round_bound[r]) * kPageSlots)) {
                (void)hipStreamSynchronize(s);
                return DINT_ERR_HIP;
            }
            const round_tail t = tail_of_round(r, r + 1 == rounds, host_counts);
            st = decode_pages_lean(qi, t.touched, ctrl, round_bound[r], qi->probe.p, ctrl, 0u, s, nullptr, &t);
            if (st != DINT_OK) {
                (void)hipStreamSynchronize(s);
                return st;
            }
        }
        counted = true;
    }
    // The batch path: per round ONE page decode and ONE tail launch (and_round_tail_kernel: this round's probe, the release of
    // its claims, the NEXT round's block-max search) — the two rounds' claim sets alternate, as in the tail form. A round
    // in which no query has a term ends the call's rounds (a query's terms are consecutive rounds).
    for (size_t r = 0; r != rounds && !tail_form && !fused_ok; ++r) {
        const uint32_t* first = d_term_first + r * n_queries;
        const uint32_t* nblk = d_term_blocks + r * n_queries;
        uint32_t* const ctrl = d_ctrl + (r + 1) * kCtrlWords;
        uint64_t list_blocks = 0;
        for (size_t q = 0; q != n_queries; ++q) list_blocks += h_blocks[r * n_queries + q];
        if (list_blocks == 0) break;  // no query has a term for this round (nor for any later one)
        size_t bound = size_t(std::min<uint64_t>(n_slots, list_blocks));
        if (r == 0 && !searched0)
            hipLaunchKernelGGL(and_search_kernel, dim3(slot_grid), dim3(tb), 0, s, qi->cand.p, n_slots, d_page_query,
                               first, nblk, qi->d_block_max, qi->target.p, qi->d_needed, qi->d_rank, qi->d_touched, ctrl);
        const uint32_t* d_count = ctrl;
        bool nothing_touched = false;
        if (!sized_by_bound(bound, {{&qi->probe, bound * kPageSlots}})) {
            uint32_t n_touched = 0;
            HIP_TRY(hipMemcpyAsync(&n_touched, ctrl, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            nothing_touched = n_touched == 0;  // (every candidate of the round's queries died in the search: the tail still runs)
            bound = std::max<uint32_t>(1, n_touched);
            d_count = nothing_touched ? ctrl : nullptr;
        }
        if (!qi->probe.ensure(uint64_t(bound) * kPageSlots)) {
            (void)hipStreamSynchronize(s);
            return DINT_ERR_HIP;
        }
        if (!nothing_touched) {
            st = decode_pages_counted(qi, qi->d_touched + (r & 1) * nb, d_count, bound, qi->probe.p, ctrl, 0u, s);
            if (st != DINT_OK) {
                (void)hipStreamSynchronize(s);
                return st;
            }
        }
        const round_tail t = tail_of_round(r, r == last_round, host_counts);
        counted = counted || r == last_round;
        hipLaunchKernelGGL(and_round_tail_kernel, dim3(slot_grid), dim3(tb), 0, s, t);
    }
    results_to_host = results_to_host && counted;
    if (!counted) hipLaunchKernelGGL(and_count_kernel, dim3(slot_grid), dim3(tb), 0, s, qi->cand.p, n_slots, d_page_query, d_counts);
    HIP_TRY(hipGetLastError());
    // ---- and_query<true> (queries.hpp:72-76): the freq of every term at every match. Lazily, like the reference's
    // freq(): a freqs part is decoded only for the blocks that hold a match — term by term, the blocks the
    // matches fall into (for the rarest term: the candidate pages themselves), their docs and freqs parts, then
    // every match reads its freq at the position of its docID.
    std::vector<unsigned long long> h_sums;
    std::vector<uint32_t> h_freq_counts;
    std::vector<float> h_qweights;
    if (freqs_dict) {
        if (!qi->freq_sums.ensure(n_queries)) return DINT_ERR_HIP;
        HIP_TRY(hipMemsetAsync(qi->freq_sums.p, 0, n_queries * sizeof(unsigned long long), s));
        // (the blocks a term's matches fall into are counted on the device; the launches of a term are sized for what
        // the host knows — no more blocks than matches can exist, than the terms' lists hold, than the candidate pages for
        // the rarest term — and the pages past the count are empty. Past kAsyncPages the count is read back after all,
        // as in the rounds above. The counts themselves travel to the host with the results.)
        if (!qi->freq_counts.ensure(rounds + 1)) return DINT_ERR_HIP;
        HIP_TRY(hipMemsetAsync(qi->freq_counts.p, 0, (rounds + 1) * 4, s));
        if (rk) {  // ranked_and: a score per candidate slot, from 0.0f; [j * n_queries + q] = q_weight of query q's j-th term
            h_qweights.assign((rounds + 1) * n_queries, 0.0f);
            for (size_t q = 0; q != n_queries; ++q)
                for (uint32_t j = 0; j != plan.len[q]; ++j)
                    h_qweights[j * n_queries + q] = bm25_query_term_weight(plan.qf_of(q)[j], qi->list_len[plan.of(q)[j]], rk->num_docs);
            if (!qi->slot_score.ensure(n_slots) || !qi->slot_kden.ensure(n_slots) || !qi->qweights.ensure(h_qweights.size()))
                return DINT_ERR_HIP;
            HIP_TRY(hipMemsetAsync(qi->slot_score.p, 0, n_slots * sizeof(float), s));
            HIP_TRY(hipMemcpyAsync(qi->qweights.p, h_qweights.data(), h_qweights.size() * sizeof(float), hipMemcpyHostToDevice, s));
        }
        for (size_t r = 0; r != rounds + 1; ++r) {  // r = 0: the rarest term; r >= 1: the term of round r - 1
            const uint32_t* first = r ? d_term_first + (r - 1) * n_queries : nullptr;
            const uint32_t* nblk = r ? d_term_blocks + (r - 1) * n_queries : nullptr;
            uint64_t list_blocks = n_pages;
            if (r) {
                list_blocks = 0;
                for (size_t q = 0; q != n_queries; ++q) list_blocks += h_blocks[(r - 1) * n_queries + q];
            }
            size_t bound = size_t(std::min<uint64_t>(n_slots, list_blocks));
            if (bound == 0) continue;
            uint32_t* const d_cnt = qi->freq_counts.p + r;
            hipLaunchKernelGGL(and_freq_search_kernel, dim3(slot_grid), dim3(tb), 0, s, qi->cand.p, n_slots, d_page_query,
                               d_page_block, first, nblk, qi->d_block_max, qi->target.p, qi->d_needed, qi->d_rank,
                               qi->d_touched, d_cnt);
            const uint32_t* d_count = d_cnt;
            if (!sized_by_bound(bound, {{&qi->probe, bound * kPageSlots}, {&qi->fprobe, bound * kPageSlots}})) {
                uint32_t n_touched = 0;
                HIP_TRY(hipMemcpyAsync(&n_touched, d_cnt, 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                if (n_touched == 0) continue;
                bound = n_touched;
                d_count = nullptr;
            }
            if (!qi->sub.ensure(std::max<size_t>(n_pages, bound)) || !qi->probe.ensure(uint64_t(bound) * kPageSlots) ||
                !qi->fprobe.ensure(uint64_t(bound) * kPageSlots)) {
                (void)hipStreamSynchronize(s);
                return DINT_ERR_HIP;
            }
            const uint32_t tgrid = uint32_t((bound + tb - 1) / tb);
            hipLaunchKernelGGL(gather_pages_kernel, dim3(tgrid), dim3(tb), 0, s, qi->d_blocks, qi->d_touched, uint64_t(bound), qi->sub.p,
                               d_count);
            st = decode_pages(qi, bound, qi->probe.p, freqs_dict, qi->fprobe.p, s);
            if (st != DINT_OK) {
                (void)hipStreamSynchronize(s);
                return st;
            }
            if (rk)  // (the terms in this path's order: the score is summed in the reference's order, DESIGN.md 4d-ranked)
                hipLaunchKernelGGL(ranked_gather_kernel, dim3(slot_grid), dim3(tb), 0, s, qi->cand.p, n_slots, d_page_query, nblk,
                                   qi->d_blocks, qi->target.p, qi->d_rank, qi->probe.p, qi->fprobe.p, qi->qweights.p + r * n_queries,
                                   rk->norm_lens, qi->slot_kden.p, qi->slot_score.p);
            else
                hipLaunchKernelGGL(and_freq_gather_kernel, dim3(slot_grid), dim3(tb), 0, s, qi->cand.p, n_slots, d_page_query, nblk,
                                   qi->d_blocks, qi->target.p, qi->d_rank, qi->probe.p, qi->fprobe.p, qi->freq_sums.p);
            hipLaunchKernelGGL(and_release_kernel, dim3(tgrid), dim3(tb), 0, s, qi->d_touched, uint32_t(bound), qi->d_needed, d_count);
        }
        HIP_TRY(hipGetLastError());
        if (rk) {
            st = ranked_topk(qi, *rk, h_page_query, n_queries, s);
            if (st != DINT_OK) {
                (void)hipStreamSynchronize(s);
                return st;
            }
        }
        h_sums.resize(n_queries);
        HIP_TRY(hipMemcpyAsync(h_sums.data(), qi->freq_sums.p, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        h_freq_counts.resize(rounds + 1);
        HIP_TRY(hipMemcpyAsync(h_freq_counts.data(), qi->freq_counts.p, (rounds + 1) * 4, hipMemcpyDeviceToHost, s));
    }
    unsigned long long* const h_counts = static_cast<unsigned long long*>(qi->h_stage);  // (the inputs have long been copied)
    if (!results_to_host) HIP_TRY(hipMemcpyAsync(h_counts, d_counts, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    // (Watching a flag in pinned memory, written behind the results, instead of the stream was measured: no faster.)
    HIP_TRY(hipStreamSynchronize(s));
    qi->claims_dirty = false;
    for (size_t q = 0; q != n_queries; ++q)
        if (plan.len[q] != 0) counts[q] = h_counts[q];
    if (freqs_dict) {
        for (size_t q = 0; q != n_queries; ++q) freq_sums[q] = h_sums[q];
        if (freq_blocks)
            for (uint32_t c : h_freq_counts) *freq_blocks += c;
    }
    return DINT_OK;
}

