// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": disjunctive queries (queries.hpp:86-130).
// ---- disjunctive queries ------------------------------------------------------------------------
// or_query visits every docID some list of the query holds, once, and (with_freqs) reads the freq of every posting: every
// block of every distinct term is decoded, so there is nothing to skip and nothing to claim. A call is cut into passes of
// whole queries of at most DINT_OPT_QUERY_OR_PASS_PAGES pages; per pass one copy in, the pages' decode (decode_pages, as
// the AND path decodes its freqs pages) and ONE probe launch (or_count_kernel, dint_or_query_kernels.hpp) that adds to the
// call's counters. The counters come back once, at the end. The claim flags and tables of the AND forms are not touched.
// rk (dint_ranked_or_queries, hip_api_ranked_or_query.inc): the pass's probe launch is ranked_or_score_kernel instead, and
// ranked_topk writes the best keys of the pass's queries to rk->keys at their own offset; the counters are not used.
// xb (dint_ranked_or_bool_queries, hip_api_ranked_or_bool.inc), with rk: the scoring launch is ranked_or_bool_score_kernel,
// which also drops the documents in fewer than m lists; the excluded terms' steps (bool_step) and and_count_kernel run
// between it and ranked_topk, and the counters come back with the last pass. Without xb nothing is launched differently.
// rg (dint_ranked_or_range_queries, hip_api_ranked_range.inc), with rk: the pages are the blocks in every query's docID range
// only, the scoring launch is ranked_or_range_score_kernel, which counts the matches into the call's counters, and those
// come back with the last pass. Without rg nothing is planned or launched differently.
// fl (dint_ranked_or_filtered_queries, hip_api_doc_filter.inc), with rk and without rg: the pages are every term's LIVE blocks
// under the call's filter, the term records still describe the whole lists, the scoring launch is
// ranked_or_filtered_score_kernel, which finds a block's page through the filter's live rank and counts the matches into
// the call's counters; those come back with the last pass. Without fl nothing is planned or launched differently.
// x (the faceted, collapsed, paged, group-limited, sorted, value-stats, group-stats, percentile and top-values entries), with rk and with
// rg or fl: its workspaces are cleared once per call, a pass stages its page -> query table besides and runs x's launches in
// front of ranked_topk and behind it, over the pass's slots in cand at the pass's query offset — a pass holds whole queries,
// so a query's slots are complete — and its results come back with the last pass (ranked_extras: the steps and their order).
// Without any nothing is planned or launched differently.

// What a ranked OR call with a minimum and exclusions adds to its passes, and what it gets back.
struct or_bool_args {
    const uint32_t* m = nullptr;           // per query: the distinct optional terms whose list must hold a match (>= 1)
    std::vector<uint32_t> not_terms;       // every query's distinct excluded terms, ascending: query q's at [not_at[q], not_at[q + 1])
    std::vector<uint64_t> not_at;          // n_queries + 1
    uint64_t eager_blocks = 0;             // out: the blocks the passes decode before any step
    std::vector<std::vector<uint32_t>> step_claims;  // out: per pass with steps, per step the blocks it claimed
    std::vector<unsigned long long> h_matches;       // out: the call's counters (a query the call did not run: 0)
    bool claimed = false;  // a pass of this call has run a step: the handle's claims_dirty is this call's to clear at its end
};

// The set-up of an OR call, shared with the pruned ranked call (hip_api_ranked_or_maxscore.inc): the plan (longest list
// first, with multiplicities if with_qf), every query's pages (every block of its distinct terms; a query without any
// has len 0, and so has one of fewer distinct terms than its min_match) and the passes: whole queries, at most `limit`
// pages each — a query larger than that alone, in a pass sized to it.
struct or_passes {
    query_plan plan;
    std::vector<uint64_t> pages;  // per query
    std::vector<size_t> first;    // pass k: queries [first[k], first[k + 1])
    uint64_t all = 0;
};
static int plan_or_passes(const dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                          bool with_qf, bool with_freqs, uint64_t* counts, uint64_t* freq_sums, or_passes& op,
                          const uint32_t* min_match = nullptr, const range_args* rg = nullptr, const filter_args* fl = nullptr) {
    query_plan& plan = op.plan;
    const int planned = plan_queries(qi, terms, query_offsets, n_queries, true, with_qf, with_freqs, counts, freq_sums, plan);
    if (planned != DINT_OK) return planned;
    op.pages.assign(n_queries, 0);
    op.all = 0;
    for (size_t q = 0; q != n_queries; ++q) {
        for (uint32_t j = 0; j != plan.len[q]; ++j) op.pages[q] += planned_blocks(qi, plan.of(q)[j], rg ? &rg->ranges[q] : nullptr, fl);
        if (op.pages[q] == 0) plan.len[q] = 0;  // (lists without a block, or without one in the query's range / live under the filter)
        if (min_match && min_match[q] > plan.len[q]) plan.len[q] = 0, op.pages[q] = 0;  // (more lists asked for than the query has)
        op.all += op.pages[q];
    }
    op.first = cut_passes(n_queries, {{op.pages.data(), uint64_t(opt(DINT_OPT_QUERY_OR_PASS_PAGES))}}, false);
    return DINT_OK;
}

// One pass: every block of the terms of its queries decoded, then ONE probe launch. A query of the pass as the pass
// sees it: the id its records carry, its terms (longest list first) and, ranked, their multiplicities.
struct or_pass_query {
    uint32_t id, n;
    const uint32_t *terms, *qf;
    const dint_doc_range* range = nullptr;  // (a ranged call: the query's; else none)
};
// The pass of `qs` on the stream: the inputs (or_pass_layout) staged — in an area
// of at least min_stage bytes — and copied in, the pages' decode, and or_count_kernel, which adds to d_counts and the
// sums behind them; or (rk) ranked_or_score_kernel over the union's representatives and ranked_topk, which selects the
// best rk->k of the queries id0 .. id0 + n_ids - 1 into rk->keys. No wait. xb (with rk and d_counts): or_bool_layout staged
// behind the pass's own; between the scoring and the selection, per excluded term of the pass's queries in ascending term
// id a step over the pass's slots (bool_step: search, claim, the docs parts decoded into qi->probe — the scoring has read
// the pass's pages by then —, the candidates found killed, release), then and_count_kernel into d_counts from id0 on.
// ranged (with rk and d_counts; every query of qs has its range): a term record's blocks are its list's blocks in range,
// or_range_layout staged behind the pass's own, and ranked_or_range_score_kernel scores, adding the matches to d_counts.
// fl (with rk and d_counts, not ranged): a term record's pages are its list's live blocks, the record itself the whole
// list's; nothing more is staged, and ranked_or_filtered_score_kernel scores, adding the matches to d_counts.
// x (with rk; its workspaces cleared): or_facet_layout staged behind the others where x wants the page -> query table;
// x.before_selection behind the scoring launch and xb's steps, x.after_selection behind the selection.
static int or_run_pass(dint_query_index* qi, const dint_dict* freqs_dict, const ranked_args* rk, const std::vector<or_pass_query>& qs,
                       size_t min_stage, unsigned long long* d_counts, size_t n_counts, uint32_t id0, size_t n_ids, hipStream_t s,
                       const ranked_extras& x, or_bool_args* xb = nullptr, bool ranged = false, const filter_args* fl = nullptr) {
    uint64_t n_pages = 0, n_terms = 0;
    for (const or_pass_query& q : qs) {
        n_terms += q.n;
        for (uint32_t j = 0; j != q.n; ++j) n_pages += planned_blocks(qi, q.terms[j], q.range, fl);
    }
    const or_pass_layout L(n_pages, n_terms, rk != nullptr);
    size_t n_steps = 0;  // (xb: the most excluded terms of a query of the pass that has pages)
    if (xb)
        for (const or_pass_query& q : qs)
            if (q.n) n_steps = std::max<size_t>(n_steps, xb->not_at[q.id + 1] - xb->not_at[q.id]);
    const or_bool_layout B(L.words, xb ? n_pages : 0, xb ? n_terms : 0, n_steps * n_ids, n_steps);
    const or_range_layout R(B.words, ranged ? n_terms : 0);
    const or_facet_layout F(R.words, x.wants_page_query() ? n_pages : 0);
    const size_t up_words = F.words;  // (without xb and x's table and not ranged: L.words)
    if (qi->stage(std::max<size_t>(up_words * 4, min_stage)) != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
    uint32_t *page_block = qi->h(L.page_block), *page_term = qi->h(L.page_term), *term_order = qi->h(L.term_order);
    std::vector<uint32_t> page_query(rk ? n_pages : 0);  // (ranked_topk's: the pass's queries, from 0)
    uint32_t page = 0, rec = 0;
    for (const or_pass_query& q : qs) {
        const uint32_t from = rec;
        if (rk) sort_records_by_term(term_order, from, q.n, q.terms);
        for (uint32_t j = 0; j != q.n; ++j, ++rec) {
            const uint32_t l = q.terms[j];
            const block_span in = blocks_in_range(qi, l, q.range);  // (no range: every block of the list)
            qi->h(L.term_first)[rec] = qi->list_first[l] + in.p0;
            qi->h(L.term_blocks)[rec] = in.size();
            qi->h(L.term_page)[rec] = page;
            qi->h(L.term_query)[rec] = q.id;
            qi->h(L.term_from)[rec] = from;
            if (xb) qi->h(B.term_m)[rec] = xb->m[q.id];
            if (rk) {
                qi->h(L.term_n)[rec] = q.n;
                qi->h<float>(L.term_weight)[rec] = bm25_query_term_weight(q.qf[j], qi->list_len[l], rk->num_docs);
            }
            if (ranged) qi->h(R.term_lo)[rec] = q.range->lo, qi->h(R.term_hi)[rec] = q.range->hi;
            for (uint32_t b = qi->list_first[l] + in.p0; b != qi->list_first[l] + in.p1; ++b) {
                if (!block_planned(fl, b)) continue;  // (a filter: the live blocks only)
                page_block[page] = b;
                page_term[page] = rec;
                if (rk) page_query[page] = q.id - id0;
                ++page;
            }
        }
    }
    if (x.wants_page_query() && n_pages) std::memcpy(qi->h(F.page_query), page_query.data(), n_pages * 4);
    if (xb) {
        if (n_pages) std::memcpy(qi->h(B.page_query), page_query.data(), n_pages * 4);
        std::memset(qi->h(B.not_first), 0, (B.words - B.not_first) * 4);
        for (const or_pass_query& q : qs)
            for (uint64_t j = 0, n = q.n ? xb->not_at[q.id + 1] - xb->not_at[q.id] : 0; j != n; ++j) {
                const uint32_t l = xb->not_terms[xb->not_at[q.id] + j];
                qi->h(B.not_first)[j * n_ids + (q.id - id0)] = qi->list_first[l];
                qi->h(B.not_blocks)[j * n_ids + (q.id - id0)] = qi->blocks_of(l);
            }
    }
    if (!qi->inputs.ensure(up_words) || !qi->sub.ensure(n_pages) || !qi->probe.ensure(n_pages * kPageSlots) ||
        (freqs_dict && !qi->fprobe.ensure(n_pages * kPageSlots)))
        return stream_failed(s, DINT_ERR_HIP);
    HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, up_words * 4, hipMemcpyHostToDevice, s));
    const int st = gather_decode_pages(qi, qi->d(L.page_block), nullptr, n_pages, 0, freqs_dict, s);
    if (st != DINT_OK) return stream_failed(s, st);
    or_pass p{};
    p.page_block = qi->d(L.page_block);
    p.page_term = qi->d(L.page_term);
    p.term_first = qi->d(L.term_first);
    p.term_blocks = qi->d(L.term_blocks);
    p.term_page = qi->d(L.term_page);
    p.term_query = qi->d(L.term_query);
    p.term_from = qi->d(L.term_from);
    p.blocks = qi->d_blocks;
    p.block_max = qi->d_block_max;
    p.docs = qi->probe.p;
    p.freqs = freqs_dict ? qi->fprobe.p : nullptr;
    p.counts = d_counts;
    p.freq_sums = d_counts + n_counts;
    if (!rk) {
        hipLaunchKernelGGL(or_count_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, p);
        return hipGetLastError() != hipSuccess ? stream_failed(s, DINT_ERR_HIP) : DINT_OK;
    }
    // score the union's representatives, then select every query's best k
    if (!qi->cand.ensure(n_pages * kPageSlots) || !qi->slot_score.ensure(n_pages * kPageSlots)) return stream_failed(s, DINT_ERR_HIP);
    ranked_or_pass rp{};
    rp.base = p;
    rp.term_order = qi->d(L.term_order);
    rp.term_n = qi->d(L.term_n);
    rp.term_weight = qi->d<const float>(L.term_weight);
    rp.norm_lens = rk->norm_lens;
    rp.cand = qi->cand.p;
    rp.score = qi->slot_score.p;
    if (fl) {
        ranked_or_filtered_pass fp{};
        fp.base = rp;
        fp.filter = fl->filter->view();
        fp.matches = d_counts;
        hipLaunchKernelGGL(ranked_or_filtered_score_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, fp);
    } else if (ranged) {
        ranked_or_range_pass gp{};
        gp.base = rp;
        gp.term_lo = qi->d(R.term_lo);
        gp.term_hi = qi->d(R.term_hi);
        gp.matches = d_counts;
        hipLaunchKernelGGL(ranked_or_range_score_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, gp);
    } else if (!xb) {
        hipLaunchKernelGGL(ranked_or_score_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, rp);
    } else {
        ranked_or_bool_pass bp{};
        bp.base = rp;
        bp.term_m = qi->d(B.term_m);
        hipLaunchKernelGGL(ranked_or_bool_score_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, bp);
    }
    if (hipGetLastError() != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
    if (xb) {
        const uint64_t n_slots = n_pages * kPageSlots;
        if (n_steps) {
            if (!qi->target.ensure(n_slots)) return stream_failed(s, DINT_ERR_HIP);
            // (or_queries_impl has cleared what an earlier call may have left in the claim set, once for the call)
            qi->claims_dirty = xb->claimed = true;  // until the call has run to its end (or_queries_impl)
            const bool_slots slots{qi, nullptr, n_slots, qi->d(B.page_query), n_ids, s};
            for (size_t j = 0; j != n_steps; ++j) {
                const int xst = bool_step(slots, qi->d(B.not_first) + j * n_ids, qi->d(B.not_blocks) + j * n_ids, qi->h(B.not_blocks) + j * n_ids,
                                          nullptr, qi->d(B.step_count) + j);
                if (xst != DINT_OK) return stream_failed(s, xst);
            }
            xb->step_claims.emplace_back(n_steps, 0u);
            if (hipMemcpyAsync(xb->step_claims.back().data(), qi->d(B.step_count), n_steps * 4, hipMemcpyDeviceToHost, s) != hipSuccess)
                return stream_failed(s, DINT_ERR_HIP);
        }
        hipLaunchKernelGGL(and_count_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_slots, qi->d(B.page_query),
                           d_counts + id0);
        if (hipGetLastError() != hipSuccess) return stream_failed(s, DINT_ERR_HIP);
    }
    int rst = x.before_selection(qi, n_pages, page_query, qi->d(F.page_query), id0, n_ids, s);
    if (rst == DINT_OK) rst = ranked_topk(qi, *rk, page_query, n_ids, s, x.sv);
    if (rst == DINT_OK) rst = x.after_selection(qi, n_pages, qi->d(F.page_query), id0, n_ids, s);
    return rst != DINT_OK ? stream_failed(s, rst) : DINT_OK;
}

static int or_queries_impl(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                           size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks, void* stream, const ranked_extras& x,
                           const ranked_args* rk = nullptr, or_bool_args* xb = nullptr, range_args* rg = nullptr, filter_args* fl = nullptr) {
    if (!qi || (n_queries && (!query_offsets || !counts))) return DINT_ERR_ARG;
    if (freq_blocks) *freq_blocks = 0;
    if (n_queries == 0) return DINT_OK;
    if (n_queries >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    or_passes op;  // (rk: with multiplicities, for the query weights)
    const int planned = plan_or_passes(qi, terms, query_offsets, n_queries, rk != nullptr, freqs_dict != nullptr, counts, freq_sums, op,
                                       xb ? xb->m : nullptr, rg, fl);
    if (planned != DINT_OK) return planned;
    const query_plan& plan = op.plan;
    if (xb) {
        xb->eager_blocks = op.all;
        xb->h_matches.assign(n_queries, 0ull);
    }
    if (rg) {
        rg->blocks = op.all;
        rg->h_matches.assign(n_queries, 0ull);
    }
    if (fl) {
        fl->blocks = op.all;
        fl->h_matches.assign(n_queries, 0ull);
    }
    x.begin(n_queries);
    if (op.all == 0) return DINT_OK;

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int cleared = x.clear(qi, n_queries, s);
    if (cleared != DINT_OK) return cleared;
    // the call's counters: counts[n_queries] then freq sums[n_queries], cleared once, added to by every pass
    if (!qi->freq_sums.ensure(2 * n_queries)) return DINT_ERR_HIP;
    unsigned long long* const d_counts = qi->freq_sums.p;
    HIP_TRY(hipMemsetAsync(d_counts, 0, 2 * n_queries * sizeof(unsigned long long), s));
    // xb with excluded terms: its steps claim in the handle's dense claim set — cleared here, once for the call, of what a
    // call that failed between a search and its release left behind (and_send_inputs). A call without steps leaves the
    // flag and the set alone.
    if (xb && !xb->not_terms.empty() && qi->claims_dirty) {
        HIP_TRY(hipMemsetAsync(qi->d_needed, 0, 2 * std::max<size_t>(1, qi->n_blocks) * 4, s));
        qi->claims_dirty = false;
    }
    std::vector<or_pass_query> qs;
    for (size_t k = 0; k + 1 < op.first.size(); ++k) {
        const size_t q0 = op.first[k], q1 = op.first[k + 1];
        uint64_t n_pages = 0;
        qs.clear();
        for (size_t q = q0; q != q1; ++q) {
            n_pages += op.pages[q];
            qs.push_back({uint32_t(q), plan.len[q], plan.of(q), rk ? plan.qf_of(q) : nullptr, rg ? &rg->ranges[q] : nullptr});
        }
        if (n_pages == 0) continue;
        if (k != 0) HIP_TRY(hipStreamSynchronize(s));  // (the last pass's inputs have left the staging area)
        ranked_args pass_rk = rk ? *rk : ranked_args{};
        if (rk) pass_rk.keys += uint64_t(q0) * rk->k;  // (the keys of the pass's queries at their own offset)
        const int st = or_run_pass(qi, freqs_dict, rk ? &pass_rk : nullptr, qs, 2 * n_queries * sizeof(unsigned long long), d_counts,
                                   n_queries, uint32_t(q0), q1 - q0, s, x, xb, rg != nullptr, fl);
        if (st != DINT_OK) return st;
    }
    const int back = x.back(n_queries, s);
    if (back != DINT_OK) return back;
    if (fl) HIP_TRY(hipMemcpyAsync(fl->h_matches.data(), d_counts, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (rg) HIP_TRY(hipMemcpyAsync(rg->h_matches.data(), d_counts, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (xb) HIP_TRY(hipMemcpyAsync(xb->h_matches.data(), d_counts, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the last pass's inputs have left the staging area: the results go there)
    if (xb && xb->claimed) qi->claims_dirty = false;  // (this call set it, and every step's claims are released)
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
                if (freq_blocks) *freq_blocks += op.pages[q];
            }
        }
    return DINT_OK;
}

int dint_or_queries(dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                    uint64_t* counts, void* stream) {
    return or_queries_impl(qi, nullptr, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream, ranked_extras());
}

int dint_or_queries_freqs(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                          size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks_decoded, void* stream) {
    if (!freqs_args_ok(qi, freqs_dict, freq_sums)) return DINT_ERR_ARG;
    return or_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums, freq_blocks_decoded, stream, ranked_extras());
}
