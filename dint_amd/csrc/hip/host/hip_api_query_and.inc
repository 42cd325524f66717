// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": conjunctive queries (queries.hpp:34-84).
// ---- conjunctive queries ------------------------------------------------------------------------

// A ranked boolean call's steps behind the AND rounds (hip_api_ranked_bool.inc): per step j and query q, at
// [j * n_queries + q], the first block and the block count of the query's j-th excluded / optional term in ascending term
// id (0 blocks: the query has fewer terms, or the list is empty) and the optional term's q_weight. Once staged
// (bool_stage_steps): the tables and a claim counter per step on the device; at the end h_claims, the counters' values.
struct bool_steps {
    std::vector<uint32_t> not_first, not_blocks, should_first, should_blocks;
    std::vector<float> should_weight;
    size_t n_not = 0, n_should = 0;  // steps: the most excluded / optional terms of a query
    const uint32_t *d_not_first = nullptr, *d_not_blocks = nullptr, *d_should_first = nullptr, *d_should_blocks = nullptr;
    const float* d_should_weight = nullptr;
    uint32_t* d_step_count = nullptr;  // [0, n_not): the excluded steps, then the optional ones
    std::vector<uint32_t> h_claims;
};

static int and_queries_impl(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                            size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks, void* stream, const ranked_extras& x,
                            bool may_split = true, const ranked_args* rk = nullptr, bool_steps* extra = nullptr, range_args* rg = nullptr,
                            filter_args* fl = nullptr);

// One AND call: what its stages share.
struct and_call {
    dint_query_index* qi = nullptr;
    const dint_dict* freqs_dict = nullptr;  // and_query<true>: the freqs pass runs
    const ranked_args* rk = nullptr;        // ranked_and: the freqs pass scores and selects
    bool_steps* extra = nullptr;            // ranked_bool: excluded steps before the freqs pass, optional steps inside it
    range_args* rg = nullptr;               // a ranged call: candidates from the rarest list's blocks in range, the others killed
    filter_args* fl = nullptr;              // a filtered call: candidates from the rarest list's live blocks, the others killed
    ranked_extras x;                        // (ranked) what runs around the selection besides: the five steps of ranked_extras
    size_t n_queries = 0;
    uint64_t* counts = nullptr;
    hipStream_t s = nullptr;
    query_plan plan;
    std::vector<uint32_t> page_block, page_query;   // per candidate page: its block, its query (the rarest list of every query)
    std::vector<uint32_t> term_first, term_blocks;  // [r * n_queries + q]: first block and block count of query q's list of round r
    size_t rounds = 0, n_pages = 0;
    uint64_t n_slots = 0;
    // the general form, once staged (and_stage_general): the tables and counters on the device, and a bound of the pages
    // each round decodes (0: no query has a term for the round)
    uint32_t *d_page_block = nullptr, *d_page_query = nullptr, *d_term_first = nullptr, *d_term_blocks = nullptr, *d_ctrl = nullptr;
    unsigned long long* d_counts = nullptr;
    size_t steps_at = 0, up_words = 0;
    std::vector<size_t> round_bound;
    bool small_rounds = false;
    bool results_to_host = false;  // the last probe has written the results to the staging area itself
    // the freqs pass's results, on their way back with the counts
    std::vector<unsigned long long> h_sums;
    std::vector<uint32_t> h_freq_counts;
    std::vector<float> h_qweights;
    std::vector<uint32_t> h_ranges;  // a ranged call: per query {lo, hi}, on their way in (the call waits before it returns)

    uint32_t* ctrl_of_round(size_t r) const { return d_ctrl + (r + 1) * kCtrlWords; }  // (d_ctrl itself: the candidates' decode)
    uint32_t slot_grid() const { return uint32_t(n_pages); }                           // 256 slots per page = one workgroup
    int failed(int st) const { return stream_failed(s, st); }
};

// a query of a few candidate pages (the workgroup-per-query launch takes it)
static bool small_query(const and_call& c, size_t q) { return c.qi->blocks_of(c.plan.of(q)[0]) <= kBatchPages; }

// some list of the call holds a full block (else nothing reads the dictionary's image: query_decode_args)
static bool any_full_block(const and_call& c) {
    for (size_t q = 0; q != c.n_queries; ++q)
        for (uint32_t j = 0; j != c.plan.len[q]; ++j)
            if (c.qi->list_len[c.plan.of(q)[j]] >= kBlock) return true;
    return false;
}

// the extra steps (hip_api_ranked_bool.inc): staged with the call's inputs; the excluded terms' steps and the recount
// behind the AND rounds; the optional terms' steps behind the freqs pass's required terms
static void bool_stage_steps(and_call& c, const and_bool_layout& L);
static int bool_exclude_pass(and_call& c);
static int bool_should_pass(and_call& c);
// What a step of either clause runs over (bool_step, hip_api_ranked_bool.inc): the candidate slots in qi->cand, 256 to a
// page, a page to a query — of this call, or of an OR pass (hip_api_or_query.inc).
struct bool_slots {
    dint_query_index* qi;
    const dint_dict* freqs_dict;  // (what an optional step decodes freqs parts with)
    uint64_t n_slots;
    const uint32_t* d_page_query;  // device: page -> query, the index into the step's rows
    size_t n_queries;              // ... and the rows' length
    hipStream_t s;
    uint32_t slot_grid() const { return uint32_t(n_slots / kPageSlots); }
};
static int bool_step(const bool_slots& b, const uint32_t* first, const uint32_t* nblk, const uint32_t* h_nblk, const float* weight,
                     uint32_t* d_cnt);

// the candidates: the rarest list of every query, a page per block (a ranged call: per block in the query's range; a
// filtered call: per live block)
static void and_candidate_pages(and_call& c) {
    c.page_block.reserve(c.n_queries + 64);
    c.page_query.reserve(c.n_queries + 64);
    for (size_t q = 0; q != c.n_queries; ++q) {
        if (c.plan.len[q] == 0) continue;
        c.rounds = std::max<size_t>(c.rounds, c.plan.len[q] - 1);
        const uint32_t rarest = c.plan.of(q)[0];
        const block_span in = blocks_in_range(c.qi, rarest, c.rg ? &c.rg->ranges[q] : nullptr);
        for (uint32_t b = c.qi->list_first[rarest] + in.p0; b != c.qi->list_first[rarest] + in.p1; ++b) {
            if (!block_planned(c.fl, b)) continue;
            c.page_block.push_back(b);
            c.page_query.push_back(uint32_t(q));
        }
    }
    c.n_pages = c.page_block.size();
    c.n_slots = uint64_t(c.n_pages) * kPageSlots;
}

static void and_round_tables(and_call& c) {
    c.term_first.assign(std::max<size_t>(1, c.rounds * c.n_queries), 0);
    c.term_blocks.assign(std::max<size_t>(1, c.rounds * c.n_queries), 0);
    for (size_t q = 0; q != c.n_queries; ++q)
        for (size_t j = 1; j < c.plan.len[q]; ++j) {
            const uint32_t l = c.plan.of(q)[j];
            c.term_first[(j - 1) * c.n_queries + q] = c.qi->list_first[l];
            c.term_blocks[(j - 1) * c.n_queries + q] = c.qi->blocks_of(l);
        }
}

// the four tables into the staging area (both layouts begin with them)
static void and_stage_tables(const and_call& c, const and_tables_layout& L) {
    std::memcpy(c.qi->h(L.page_block), c.page_block.data(), c.n_pages * 4);
    std::memcpy(c.qi->h(L.page_query), c.page_query.data(), c.n_pages * 4);
    std::memcpy(c.qi->h(L.term_first), c.term_first.data(), c.term_first.size() * 4);
    std::memcpy(c.qi->h(L.term_blocks), c.term_blocks.data(), c.term_blocks.size() * 4);
}

// A MIXED call — queries of a few candidate pages among queries of hundreds: the small ones go through the
// workgroup-per-query launch, the others through the round-per-launch form, as two calls of and_queries_impl over the
// sorted plans (a single large query no longer takes a log of small ones onto the slow form with it).
static int and_mixed_split(const and_call& c, void* stream, bool* mixed) {
    size_t n_small = 0, n_large = 0;
    for (size_t q = 0; q != c.n_queries; ++q)
        if (c.plan.len[q] != 0) (small_query(c, q) ? n_small : n_large) += 1;
    *mixed = !c.freqs_dict && c.n_queries >= 3 && opt(DINT_OPT_QUERY_BATCH_FUSED) != 0 && n_small >= 2 && n_large != 0;
    if (!*mixed) return DINT_OK;
    for (int part = 0; part != 2; ++part) {  // 0: the small queries, 1: the others
        std::vector<uint32_t> sub_terms, sub_q;
        std::vector<uint64_t> sub_offs(1, 0);
        for (size_t q = 0; q != c.n_queries; ++q) {
            if (c.plan.len[q] == 0 || small_query(c, q) != (part == 0)) continue;
            sub_terms.insert(sub_terms.end(), c.plan.of(q), c.plan.of(q) + c.plan.len[q]);
            sub_offs.push_back(sub_terms.size());
            sub_q.push_back(uint32_t(q));
        }
        std::vector<uint64_t> sub_counts(sub_q.size(), 0);
        const int st = and_queries_impl(c.qi, nullptr, sub_terms.data(), sub_offs.data(), sub_q.size(), sub_counts.data(), nullptr, nullptr, stream,
                                        ranked_extras(), false);
        if (st != DINT_OK) return st;
        for (size_t k = 0; k != sub_q.size(); ++k) c.counts[sub_q[k]] = sub_counts[k];
    }
    return DINT_OK;
}

// ---- a call of SMALL queries (a few candidate pages each — the reference's log): a workgroup per query, ONE launch
// (query_batch_body; DINT_OPT_QUERY_BATCH_FUSED = 0: the round-per-launch batch form below, as until late in round 5) ----
struct and_batch_plan {
    std::vector<uint32_t> rec;  // per active query: {query, first page, pages, steps} then {probe page, control word}
    uint64_t probe_pages = 0, ctrl_at = 0;
    size_t n_active() const { return rec.size() / 6; }
};
// whether the call is one for this form, and its records
static bool and_batch_fits(const and_call& c, and_batch_plan& bp) {
    const dint_query_index* qi = c.qi;
    bool small = !c.freqs_dict && c.n_queries >= 2 && c.rounds != 0 && qi->index_bytes >= 8 && opt(DINT_OPT_QUERY_BATCH_FUSED) != 0 &&
                 c.n_pages < 0xFFFFFFFFull / kPageSlots;
    if (!small) return false;
    bp.rec.reserve(6 * c.n_queries);
    size_t page = 0;
    for (size_t q = 0; q != c.n_queries && small; ++q) {
        if (c.plan.len[q] == 0) continue;
        const uint32_t pages_q = qi->blocks_of(c.plan.of(q)[0]);
        small = small_query(c, q) && c.plan.len[q] >= 2;
        uint64_t most = 0;
        for (uint32_t j = 1; j != c.plan.len[q]; ++j) most = std::max<uint64_t>(most, c.term_blocks[(j - 1) * c.n_queries + q]);
        const uint64_t stretch = std::min<uint64_t>(most, uint64_t(pages_q) * kPageSlots);
        bp.rec.insert(bp.rec.end(), {uint32_t(q), uint32_t(page), pages_q, c.plan.len[q], uint32_t(bp.probe_pages), uint32_t(bp.ctrl_at)});
        page += pages_q;
        bp.probe_pages += stretch;
        bp.ctrl_at += uint64_t(c.plan.len[q]) * kBatchCtrlWords;
        small = small && bp.probe_pages < (1ull << 22) && bp.ctrl_at < (1ull << 30);
    }
    return small && bp.n_active() != 0;
}
// the form itself, the staging area (L) at hand and mapped: in, the launch, the wait; the kernel writes the results to
// the host itself
static int and_batch_form(and_call& c, const and_batch_plan& bp, const and_batch_layout& L) {
    dint_query_index* qi = c.qi;
    const size_t n_active = bp.n_active();
    const uint32_t grid = uint32_t(std::min<size_t>(n_active, std::max<uint32_t>(1, qi->docs->compute_units) * kBlocksPerCU));
    // (per workgroup two hashed claim tables and two touched lists: 160 KB, whatever the index's size)
    const size_t slot_words = size_t(grid) * 2 * kBatchClaimSlots, touched_words = size_t(grid) * 2 * kBatchTouched;
    if (!qi->inputs.ensure(L.words + 4) || !qi->cand.ensure(c.n_slots) || !qi->target.ensure(c.n_slots) ||
        !qi->probe.ensure(std::max<uint64_t>(1, bp.probe_pages) * kPageSlots) || !qi->gaps_left.ensure(c.n_pages + bp.probe_pages + 1) ||
        !qi->batch_ctrl.ensure(std::max<uint64_t>(1, bp.ctrl_at)) || !qi->slot_rank.ensure(slot_words) || !qi->slot_touched.ensure(touched_words))
        return DINT_ERR_HIP;
    if (qi->slot_needed.cap < slot_words) qi->slot_needed_clean = 0;  // (ensure() below hands out a new, unwritten buffer)
    if (!qi->slot_needed.ensure(slot_words)) return DINT_ERR_HIP;
    if (qi->slot_needed_clean < qi->slot_needed.cap || qi->slots_dirty) {
        HIP_TRY(hipMemsetAsync(qi->slot_needed.p, 0, qi->slot_needed.cap * 4, c.s));
        qi->slot_needed_clean = qi->slot_needed.cap;
        qi->slots_dirty = false;
    }
    and_stage_tables(c, L);
    std::memset(qi->h(L.counts), 0, (L.qrec - L.counts) * 4);
    for (size_t k = 0; k != n_active; ++k) {
        std::memcpy(qi->h(L.qrec) + 4 * k, &bp.rec[6 * k], 16);
        std::memcpy(qi->h(L.qrec2) + 2 * k, &bp.rec[6 * k + 4], 8);
    }
    HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, L.words * 4, hipMemcpyHostToDevice, c.s));
    fused_batch b{};
    b.page_block = qi->d(L.page_block);
    b.page_query = qi->d(L.page_query);
    b.term_first = qi->d(L.term_first);
    b.term_blocks = qi->d(L.term_blocks);
    b.n_queries = uint32_t(c.n_queries);
    b.n_active = uint32_t(n_active);
    b.block_max = qi->d_block_max;
    b.blocks = qi->d_blocks;
    b.qrec = qi->d<const u32x4>(L.qrec);
    b.qrec2 = qi->d<const u32x2>(L.qrec2);
    b.cand = qi->cand.p;
    b.target = qi->target.p;
    b.probe = qi->probe.p;
    b.gaps_left = qi->gaps_left.p;
    b.probe_flags_at = c.n_pages;
    b.ctrl = qi->batch_ctrl.p;
    b.needed = qi->slot_needed.p;
    b.rank = qi->slot_rank.p;
    b.touched = qi->slot_touched.p;
    b.counts = qi->d<unsigned long long>(L.counts);
    b.host_counts = static_cast<unsigned long long*>(qi->d_stage);
    qi->slots_dirty = true;  // until the call has run to its end
    const int st = query_decode_launch(qi, query_decode_args(qi, any_full_block(c)), grid, c.s, decode_single_query_batch_kernel,
                                       decode_multi_query_batch_kernel, b);
    if (st != DINT_OK) return st;
    HIP_TRY(hipStreamSynchronize(c.s));
    qi->slots_dirty = false;
    const unsigned long long* const h_counts = static_cast<const unsigned long long*>(qi->h_stage);
    for (size_t q = 0; q != c.n_queries; ++q)
        if (c.plan.len[q] != 0) c.counts[q] = h_counts[q];
    return DINT_OK;
}

// ---- the general form: staging. The inputs (and_general_layout) into the staging area — d_stage: the last probe
// writes the results there —, the workspaces every form needs, and what the host knows of the rounds before anything
// runs: a bound of the pages each decodes (the live candidates at most, and no more blocks than the round's lists have) ----
static int and_stage_general(and_call& c) {
    dint_query_index* qi = c.qi;
    const bool_steps* const x = c.extra;  // (none: and_general_layout itself)
    const and_bool_layout L(c.n_pages, c.term_first.size(), c.n_queries, c.rounds, kCtrlWords, sizeof(fused_step), x ? x->not_first.size() : 0,
                            x ? x->should_first.size() : 0, x ? x->n_not + x->n_should : 0);
    HIP_TRY(qi->stage(std::max(L.words * 4, c.n_queries * sizeof(unsigned long long))));
    if (!qi->inputs.ensure(L.words + 4) || !qi->cand.ensure(c.n_slots) || !qi->target.ensure(c.n_slots)) return DINT_ERR_HIP;
    and_stage_tables(c, L);
    if (c.extra) bool_stage_steps(c, L);
    std::memset(qi->h(L.ctrl), 0, (L.steps - L.ctrl) * 4);
    c.d_page_block = qi->d(L.page_block);
    c.d_page_query = qi->d(L.page_query);
    c.d_term_first = qi->d(L.term_first);
    c.d_term_blocks = qi->d(L.term_blocks);
    c.d_ctrl = qi->d(L.ctrl);
    c.d_counts = qi->d<unsigned long long>(L.counts);
    c.steps_at = L.steps;
    c.up_words = L.words;
    c.round_bound.assign(c.rounds, 0);
    c.small_rounds = c.rounds != 0 && c.n_pages < lean_pages() && qi->index_bytes >= 8;
    for (size_t r = 0; r != c.rounds; ++r) {
        uint64_t list_blocks = 0;
        for (size_t q = 0; q != c.n_queries; ++q) list_blocks += c.term_blocks[r * c.n_queries + q];
        c.round_bound[r] = size_t(std::min<uint64_t>(c.n_slots, list_blocks));
        c.small_rounds = c.small_rounds && list_blocks != 0 && c.round_bound[r] < lean_pages();
    }
    return DINT_OK;
}

// Round r's tail (and_round_tail_kernel, or a one-launch form's step): its probe, the release of its claims, and then
// either the next round's block-max search — the two rounds' claim sets alternate — or (last) the count of the
// survivors, also written to host_counts unless that is null. Its page decode counts in ctrl_of_round(r).
static round_tail and_tail_of_round(const and_call& c, size_t r, bool last, unsigned long long* host_counts) {
    const dint_query_index* qi = c.qi;
    const size_t nb = std::max<size_t>(1, qi->n_blocks), set = r & 1, next_set = set ^ 1;
    round_tail t{};
    t.done = c.ctrl_of_round(r) + 2;  // (not counted in: non-null says "this step has a tail")
    t.cand = qi->cand.p;
    t.n_slots = c.n_slots;
    t.page_query = c.d_page_query;
    t.blocks = qi->d_blocks;
    t.target = qi->target.p;
    t.term_blocks = c.d_term_blocks + r * c.n_queries;
    t.rank = qi->d_rank + set * nb;
    t.probe = qi->probe.p;
    t.touched = qi->d_touched + set * nb;
    t.n_touched = c.ctrl_of_round(r);
    t.needed = qi->d_needed + set * nb;
    if (!last) {
        t.next_first = c.d_term_first + (r + 1) * c.n_queries;
        t.next_blocks = c.d_term_blocks + (r + 1) * c.n_queries;
        t.block_max = qi->d_block_max;
        t.next_needed = qi->d_needed + next_set * nb;
        t.next_rank = qi->d_rank + next_set * nb;
        t.next_touched = qi->d_touched + next_set * nb;
        t.next_n_touched = c.ctrl_of_round(r + 1);
    } else {
        t.counts = c.d_counts;
        t.host_counts = host_counts;
        t.n_queries = uint32_t(c.n_queries);
    }
    return t;
}

// what the first round's search, riding along the candidates' decode, needs
static query_pages and_first_search(const and_call& c) {
    query_pages sp{};
    sp.page_query = c.d_page_query;
    sp.term_first = c.d_term_first;
    sp.term_blocks = c.d_term_blocks;
    sp.block_max = c.qi->d_block_max;
    sp.target = c.qi->target.p;
    sp.needed = c.qi->d_needed;
    sp.rank = c.qi->d_rank;
    sp.touched = c.qi->d_touched;
    sp.n_touched = c.ctrl_of_round(0);
    return sp;
}

// the general form's copy in, and the clear of what a call that failed between a search and its release left behind
static int and_send_inputs(and_call& c, bool copy) {
    dint_query_index* qi = c.qi;
    if (copy) HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, c.up_words * 4, hipMemcpyHostToDevice, c.s));
    if (qi->claims_dirty) {
        HIP_TRY(hipMemsetAsync(qi->d_needed, 0, 2 * std::max<size_t>(1, qi->n_blocks) * 4, c.s));
        qi->claims_dirty = false;
    }
    return DINT_OK;
}

// ---- A query of a page or two of candidates: the whole chain — candidates, then every round's pages and tail — in ONE
// launch of one workgroup (query_fused_body; DINT_QUERY_FUSED_PAGES: at most that many candidate pages, 0: never). The
// steps are staged behind the inputs; the workgroup brings the inputs over itself — fused_inputs: no copy on the stream
// in front of it — where the staging area is mapped (DINT_OPT_QUERY_FUSED_COPY = 0: the copy after all). ----
static int and_fused_form(and_call& c) {
    dint_query_index* qi = c.qi;
    const size_t nb = std::max<size_t>(1, qi->n_blocks);
    size_t max_pages = c.n_pages;
    for (size_t r = 0; r != c.rounds; ++r) max_pages = std::max(max_pages, c.round_bound[r]);
    if (!qi->probe.ensure(uint64_t(max_pages) * kPageSlots) || !qi->gaps_left.ensure(max_pages)) return DINT_ERR_HIP;
    const bool to_host = !c.freqs_dict && qi->d_stage != nullptr;
    for (size_t k = 0; k != c.rounds + 1; ++k) {
        fused_step st{};
        st.gaps_left = qi->gaps_left.p;
        if (k == 0) {  // the candidate pages, the first round's search riding along (decode_pages_lean's candidate call)
            st.out = qi->cand.p;
            st.out_capacity = uint64_t(c.n_pages) * kPageSlots;
            st.qp = and_first_search(c);
            st.qp.ids = c.d_page_block;
            st.qp.count = nullptr;
            st.qp.bound = c.n_pages;
            st.qp.retire = 1u;
        } else {  // round r: the touched pages, then the tail (the round-tail form's round_tail)
            const size_t r = k - 1;
            st.out = qi->probe.p;
            st.out_capacity = uint64_t(c.round_bound[r]) * kPageSlots;
            st.qp.ids = qi->d_touched + (r & 1) * nb;
            st.qp.count = c.ctrl_of_round(r);
            st.qp.bound = c.round_bound[r];
            st.qp.retire = 0u;
            st.rt = and_tail_of_round(c, r, r + 1 == c.rounds, to_host ? static_cast<unsigned long long*>(qi->d_stage) : nullptr);
        }
        st.qp.blocks = qi->d_blocks;
        std::memcpy(qi->h<fused_step>(c.steps_at) + k, &st, sizeof st);
    }
    const bool bring_inputs = qi->d_stage != nullptr && opt(DINT_OPT_QUERY_FUSED_COPY) != 0;
    fused_inputs bring{};
    if (bring_inputs) {
        bring.from = static_cast<const u32x4*>(qi->d_stage);
        bring.to = reinterpret_cast<u32x4*>(qi->inputs.p);
        bring.words = uint32_t((c.up_words + 3) / 4 * 4);  // (both buffers end beyond that)
    }
    const int sent = and_send_inputs(c, !bring_inputs);
    if (sent != DINT_OK) return sent;
    const int st = query_decode_launch(qi, query_decode_args(qi, any_full_block(c)), 1, c.s, decode_single_query_fused_kernel,
                                       decode_multi_query_fused_kernel, qi->d<fused_step>(c.steps_at), uint32_t(c.rounds + 1), bring);
    if (st != DINT_OK) return st;
    qi->claims_dirty = true;  // until the call has run to its end
    return DINT_OK;
}

// ---- the other forms' beginning: the copy in; the candidates decoded, the first round's search riding along where the
// one-launch decode runs (*searched). A ranged call: no search rides along — range_kill_kernel retires the candidates
// outside their query's range behind the decode, and the first round's search is and_batch_rounds' own launch, so a
// boundary candidate claims nothing. A filtered call: the same, with filter_kill_kernel ----
static int and_candidates(and_call& c, bool* searched) {
    const int sent = and_send_inputs(c, true);
    if (sent != DINT_OK) return sent;
    const query_pages search0 = and_first_search(c);
    const int st = decode_pages_counted(c.qi, c.d_page_block, nullptr, c.n_pages, c.qi->cand.p, c.d_ctrl, 1u, c.s,
                                        !c.rg && !c.fl && c.rounds && c.round_bound[0] ? &search0 : nullptr, searched);
    if (st != DINT_OK) return c.failed(st);
    c.qi->claims_dirty = true;  // until the call has run to its end
    if (c.rg) {
        c.h_ranges.resize(2 * c.n_queries);
        for (size_t q = 0; q != c.n_queries; ++q) c.h_ranges[2 * q] = c.rg->ranges[q].lo, c.h_ranges[2 * q + 1] = c.rg->ranges[q].hi;
        if (!c.qi->q_ranges.ensure(c.h_ranges.size())) return c.failed(DINT_ERR_HIP);
        if (hipMemcpyAsync(c.qi->q_ranges.p, c.h_ranges.data(), c.h_ranges.size() * 4, hipMemcpyHostToDevice, c.s) != hipSuccess)
            return c.failed(DINT_ERR_HIP);
        hipLaunchKernelGGL(range_kill_kernel, dim3(c.slot_grid()), dim3(kPageSlots), 0, c.s, c.qi->cand.p, c.n_slots, c.d_page_query,
                           c.qi->q_ranges.p);
        if (hipGetLastError() != hipSuccess) return c.failed(DINT_ERR_HIP);
    }
    if (c.fl) {
        hipLaunchKernelGGL(filter_kill_kernel, dim3(c.slot_grid()), dim3(kPageSlots), 0, c.s, c.qi->cand.p, c.n_slots, c.fl->filter->view());
        if (hipGetLastError() != hipSuccess) return c.failed(DINT_ERR_HIP);
    }
    return DINT_OK;
}

// ---- Few candidates, few pages in every round (a single query): one launch per round — the page decode with the
// round's tail behind it (round_tail) ----
static int and_round_tail_form(and_call& c, unsigned long long* host_counts) {
    dint_query_index* qi = c.qi;
    for (size_t r = 0; r != c.rounds; ++r) {
        if (!qi->probe.ensure(uint64_t(c.round_bound[r]) * kPageSlots)) return c.failed(DINT_ERR_HIP);
        const round_tail t = and_tail_of_round(c, r, r + 1 == c.rounds, host_counts);
        const int st = decode_pages_lean(qi, t.touched, c.ctrl_of_round(r), c.round_bound[r], qi->probe.p, c.ctrl_of_round(r), 0u, c.s, nullptr, &t);
        if (st != DINT_OK) return c.failed(st);
    }
    return DINT_OK;
}

// How many blocks a round touches only the device knows; the host knows a bound and sizes the launches for that. Past
// kAsyncPages the count is read back after all — the probe buffer is sized for the bound, a kilobyte a page. (Until late
// in round 5 the limit was 32768 pages: a launch sized for a bound far above the truth cost more than the wait while
// every workgroup of it loaded the dictionary's image and swept the ticket counters; now an idle workgroup leaves at
// once, and the heavy log's call without its three mid-call waits is 3.55 against 3.68 us per query.)
constexpr size_t kAsyncPages = size_t(1) << 20;
// ... and the workspace a bound may claim on its own: a kilobyte a page, never shrunk (device_buffer). A bound that asks
// for more than this AND more than the index already owns is read back instead (4 bytes, one wait) and the buffers are
// sized for the truth; so is a bound whose allocation fails. Worst case kept by one dint_query_index for the probe pages
// (and_queries_freqs: twice, docs and freqs): max(256 MiB, 1.5 x the largest exact count seen) — include/dint_hip.h.
constexpr size_t kAsyncProbeWords = (size_t(256) << 20) / 4;
static bool sized_by_bound(size_t bound, std::initializer_list<std::pair<device_buffer<uint32_t>*, size_t>> bufs) {
    if (bound > kAsyncPages) return false;
    for (auto const& b : bufs)
        if (b.second > kAsyncProbeWords && b.second > b.first->cap) return false;
    for (auto const& b : bufs)
        if (!b.first->ensure(b.second)) {
            (void)hipGetLastError();  // (out of memory for the bound: the exact count may still fit)
            return false;
        }
    return true;
}

// ---- The batch rounds. A round: block-max search -> the touched blocks, without duplicates -> decoded -> every
// candidate probes its block. Nothing on the host waits for a round: a call is one copy in, then per round ONE page
// decode and ONE tail launch (and_round_tail_kernel: this round's probe, the release of its claims, the NEXT round's
// block-max search) — the two rounds' claim sets alternate, as in the tail form. (Round 1 read the count back every
// round and made fourteen API calls per round: a query at a time, the host's share was most of the 200 us a query
// took.) A round in which no query has a term ends the call's rounds (a query's terms are consecutive rounds). The last
// round that has anything to probe counts the survivors as well; if there is none, and_count_kernel does. ----
static int and_batch_rounds(and_call& c, bool searched0, unsigned long long* host_counts) {
    dint_query_index* qi = c.qi;
    const uint32_t tb = 256;
    const size_t nb = std::max<size_t>(1, qi->n_blocks);
    size_t last_round = c.rounds;
    for (size_t r = 0; r != c.rounds; ++r)
        if (c.round_bound[r]) last_round = r;
    bool counted = false;
    for (size_t r = 0; r != c.rounds; ++r) {
        uint32_t* const ctrl = c.ctrl_of_round(r);
        if (c.round_bound[r] == 0) break;  // no query has a term for this round (nor for any later one)
        size_t bound = c.round_bound[r];
        if (r == 0 && !searched0)
            hipLaunchKernelGGL(and_search_kernel, dim3(c.slot_grid()), dim3(tb), 0, c.s, qi->cand.p, c.n_slots, c.d_page_query, c.d_term_first,
                               c.d_term_blocks, qi->d_block_max, qi->target.p, qi->d_needed, qi->d_rank, qi->d_touched, ctrl);
        const uint32_t* d_count = ctrl;
        bool nothing_touched = false;
        if (!sized_by_bound(bound, {{&qi->probe, bound * kPageSlots}})) {
            uint32_t n_touched = 0;
            HIP_TRY(hipMemcpyAsync(&n_touched, ctrl, 4, hipMemcpyDeviceToHost, c.s));
            HIP_TRY(hipStreamSynchronize(c.s));
            nothing_touched = n_touched == 0;  // (every candidate of the round's queries died in the search: the tail still runs)
            bound = std::max<uint32_t>(1, n_touched);
            d_count = nothing_touched ? ctrl : nullptr;
        }
        if (!qi->probe.ensure(uint64_t(bound) * kPageSlots)) return c.failed(DINT_ERR_HIP);
        if (!nothing_touched) {
            const int st = decode_pages_counted(qi, qi->d_touched + (r & 1) * nb, d_count, bound, qi->probe.p, ctrl, 0u, c.s);
            if (st != DINT_OK) return c.failed(st);
        }
        const round_tail t = and_tail_of_round(c, r, r == last_round, host_counts);
        counted = counted || r == last_round;
        hipLaunchKernelGGL(and_round_tail_kernel, dim3(c.slot_grid()), dim3(tb), 0, c.s, t);
    }
    c.results_to_host = c.results_to_host && counted;
    if (!counted) hipLaunchKernelGGL(and_count_kernel, dim3(c.slot_grid()), dim3(tb), 0, c.s, qi->cand.p, c.n_slots, c.d_page_query, c.d_counts);
    return DINT_OK;
}

// ---- and_query<true> (queries.hpp:72-76): the freq of every term at every match. Lazily, like the reference's
// freq(): a freqs part is decoded only for the blocks that hold a match — term by term, the blocks the
// matches fall into (for the rarest term: the candidate pages themselves), their docs and freqs parts, then
// every match reads its freq at the position of its docID.
// (The blocks a term's matches fall into are counted on the device; the launches of a term are sized for what
// the host knows — no more blocks than matches can exist, than the terms' lists hold, than the candidate pages for
// the rarest term — and the pages past the count are empty. Past kAsyncPages the count is read back after all,
// as in the rounds above. The counts themselves travel to the host with the results.)
// rk (ranked_and): a score per candidate slot, from 0.0f, summed by ranked_gather_kernel; then ranked_topk.
// c.extra (ranked_bool): the optional terms' steps between the two; without it the launches are what they were.
// c.x (with rk): its workspaces cleared behind the optional steps, its launches in front of ranked_topk and behind it, and
// its results on their way back with the sums (ranked_extras: the steps and their order) — the call is one pass, so every
// query's slots are complete. ----
static int and_freqs_pass(and_call& c) {
    dint_query_index* qi = c.qi;
    const size_t n_queries = c.n_queries, n_terms = c.rounds + 1;
    const ranked_args* rk = c.rk;
    const uint32_t tb = 256;
    if (!qi->freq_sums.ensure(n_queries)) return DINT_ERR_HIP;
    HIP_TRY(hipMemsetAsync(qi->freq_sums.p, 0, n_queries * sizeof(unsigned long long), c.s));
    if (!qi->freq_counts.ensure(n_terms)) return DINT_ERR_HIP;
    HIP_TRY(hipMemsetAsync(qi->freq_counts.p, 0, n_terms * 4, c.s));
    if (rk) {  // [j * n_queries + q] = q_weight of query q's j-th term
        c.h_qweights.assign(n_terms * n_queries, 0.0f);
        for (size_t q = 0; q != n_queries; ++q)
            for (uint32_t j = 0; j != c.plan.len[q]; ++j)
                c.h_qweights[j * n_queries + q] = bm25_query_term_weight(c.plan.qf_of(q)[j], qi->list_len[c.plan.of(q)[j]], rk->num_docs);
        if (!qi->slot_score.ensure(c.n_slots) || !qi->slot_kden.ensure(c.n_slots) || !qi->qweights.ensure(c.h_qweights.size()))
            return DINT_ERR_HIP;
        HIP_TRY(hipMemsetAsync(qi->slot_score.p, 0, c.n_slots * sizeof(float), c.s));
        HIP_TRY(hipMemcpyAsync(qi->qweights.p, c.h_qweights.data(), c.h_qweights.size() * sizeof(float), hipMemcpyHostToDevice, c.s));
    }
    for (size_t r = 0; r != n_terms; ++r) {  // r = 0: the rarest term; r >= 1: the term of round r - 1
        const uint32_t* first = r ? c.d_term_first + (r - 1) * n_queries : nullptr;
        const uint32_t* nblk = r ? c.d_term_blocks + (r - 1) * n_queries : nullptr;
        size_t bound = r ? c.round_bound[r - 1] : c.n_pages;
        if (bound == 0) continue;
        uint32_t* const d_cnt = qi->freq_counts.p + r;
        hipLaunchKernelGGL(and_freq_search_kernel, dim3(c.slot_grid()), dim3(tb), 0, c.s, qi->cand.p, c.n_slots, c.d_page_query, c.d_page_block,
                           first, nblk, qi->d_block_max, qi->target.p, qi->d_needed, qi->d_rank, qi->d_touched, d_cnt);
        const uint32_t* d_count = d_cnt;
        if (!sized_by_bound(bound, {{&qi->probe, bound * kPageSlots}, {&qi->fprobe, bound * kPageSlots}})) {
            uint32_t n_touched = 0;
            HIP_TRY(hipMemcpyAsync(&n_touched, d_cnt, 4, hipMemcpyDeviceToHost, c.s));
            HIP_TRY(hipStreamSynchronize(c.s));
            if (n_touched == 0) continue;
            bound = n_touched;
            d_count = nullptr;
        }
        if (!qi->sub.ensure(std::max<size_t>(c.n_pages, bound)) || !qi->probe.ensure(uint64_t(bound) * kPageSlots) ||
            !qi->fprobe.ensure(uint64_t(bound) * kPageSlots))
            return c.failed(DINT_ERR_HIP);
        const int st = gather_decode_pages(qi, qi->d_touched, d_count, bound, 0, c.freqs_dict, c.s);
        if (st != DINT_OK) return c.failed(st);
        if (rk)  // (the terms in this path's order: the score is summed in the reference's order, DESIGN.md 4d-ranked)
            hipLaunchKernelGGL(ranked_gather_kernel, dim3(c.slot_grid()), dim3(tb), 0, c.s, qi->cand.p, c.n_slots, c.d_page_query, nblk,
                               qi->d_blocks, qi->target.p, qi->d_rank, qi->probe.p, qi->fprobe.p, qi->qweights.p + r * n_queries,
                               rk->norm_lens, qi->slot_kden.p, qi->slot_score.p);
        else
            hipLaunchKernelGGL(and_freq_gather_kernel, dim3(c.slot_grid()), dim3(tb), 0, c.s, qi->cand.p, c.n_slots, c.d_page_query, nblk,
                               qi->d_blocks, qi->target.p, qi->d_rank, qi->probe.p, qi->fprobe.p, qi->freq_sums.p);
        hipLaunchKernelGGL(and_release_kernel, dim3(uint32_t((bound + tb - 1) / tb)), dim3(tb), 0, c.s, qi->d_touched, uint32_t(bound),
                           qi->d_needed, d_count);
    }
    HIP_TRY(hipGetLastError());
    if (c.extra) {
        const int st = bool_should_pass(c);
        if (st != DINT_OK) return st;
    }
    if (rk) {
        int st = c.x.clear(qi, n_queries, c.s);
        if (st == DINT_OK) st = c.x.before_selection(qi, c.n_pages, c.page_query, c.d_page_query, 0u, n_queries, c.s);
        if (st == DINT_OK) st = ranked_topk(qi, *rk, c.page_query, n_queries, c.s, c.x.sv);
        if (st == DINT_OK) st = c.x.after_selection(qi, c.n_pages, c.d_page_query, 0u, n_queries, c.s);
        if (st == DINT_OK) st = c.x.back(n_queries, c.s);
        if (st != DINT_OK) return c.failed(st);
    }
    c.h_sums.resize(n_queries);
    HIP_TRY(hipMemcpyAsync(c.h_sums.data(), qi->freq_sums.p, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
    c.h_freq_counts.resize(n_terms);
    HIP_TRY(hipMemcpyAsync(c.h_freq_counts.data(), qi->freq_counts.p, n_terms * 4, hipMemcpyDeviceToHost, c.s));
    return DINT_OK;
}

// ---- the copy back: the counts (unless the last probe handed them over itself), the one wait of the call, the results
// to the caller. (Watching a flag in pinned memory, written behind the results, instead of the stream was measured: no faster.) ----
static int and_copy_back(and_call& c, uint64_t* freq_sums, uint64_t* freq_blocks) {
    dint_query_index* qi = c.qi;
    unsigned long long* const h_counts = static_cast<unsigned long long*>(qi->h_stage);  // (the inputs have long been copied)
    if (!c.results_to_host) HIP_TRY(hipMemcpyAsync(h_counts, c.d_counts, c.n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, c.s));
    HIP_TRY(hipStreamSynchronize(c.s));
    qi->claims_dirty = false;
    for (size_t q = 0; q != c.n_queries; ++q)
        if (c.plan.len[q] != 0) c.counts[q] = h_counts[q];
    if (c.freqs_dict) {
        for (size_t q = 0; q != c.n_queries; ++q) freq_sums[q] = c.h_sums[q];
        if (freq_blocks)
            for (uint32_t n : c.h_freq_counts) *freq_blocks += n;
    }
    return DINT_OK;
}

// The call: the plan, then the one place that chooses the form — mixed split, workgroup-per-query batch, fused, round
// tails or batch rounds — then, with a freqs dictionary, the freqs / ranked pass, and the copy back.
static int and_queries_impl(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                            size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks, void* stream, const ranked_extras& x,
                            bool may_split, const ranked_args* rk, bool_steps* extra, range_args* rg, filter_args* fl) {
    if (!qi || (n_queries && (!query_offsets || !counts))) return DINT_ERR_ARG;
    if (freq_blocks) *freq_blocks = 0;
    if (n_queries == 0) return DINT_OK;
    if (n_queries >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    and_call c;
    c.qi = qi;
    c.freqs_dict = freqs_dict;
    c.rk = rk;
    c.extra = extra;
    c.rg = rg;
    c.fl = fl;
    c.x = x;
    c.n_queries = n_queries;
    c.counts = counts;
    c.s = static_cast<hipStream_t>(stream);
    const int planned = plan_queries(qi, terms, query_offsets, n_queries, false, rk != nullptr, freqs_dict != nullptr, counts, freq_sums, c.plan);
    if (planned != DINT_OK) return planned;
    and_candidate_pages(c);
    if (rg) rg->blocks = c.n_pages;
    if (fl) fl->blocks = c.n_pages;
    x.begin(n_queries);
    if (c.n_pages == 0) return DINT_OK;
    bool mixed = false;
    const int split = may_split ? and_mixed_split(c, stream, &mixed) : DINT_OK;
    if (mixed) return split;
    and_round_tables(c);

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    and_batch_plan bp;
    if (and_batch_fits(c, bp)) {
        const and_batch_layout L(c.n_pages, c.term_first.size(), n_queries, bp.n_active());
        HIP_TRY(qi->stage(std::max(L.words * 4, n_queries * sizeof(unsigned long long))));
        if (qi->d_stage != nullptr) return and_batch_form(c, bp, L);
    }
    int st = and_stage_general(c);
    if (st != DINT_OK) return st;
    // (a ranged or filtered call never takes the one-launch form: its candidates die between their decode and the first search)
    const bool fused_form = !rg && !fl && c.small_rounds && c.n_pages <= tail_pages() && c.n_pages <= fused_pages();
    // the last probe hands the results over itself (a few pages: every workgroup of it passes through one counter)
    c.results_to_host = !freqs_dict && qi->d_stage != nullptr && c.n_pages <= 4096;
    unsigned long long* const host_counts = c.results_to_host ? static_cast<unsigned long long*>(qi->d_stage) : nullptr;
    if (fused_form) {
        st = and_fused_form(c);
    } else {
        bool searched0 = false;
        st = and_candidates(c, &searched0);
        const bool tail_form = searched0 && c.small_rounds && c.n_pages <= tail_pages();
        if (st == DINT_OK) st = tail_form ? and_round_tail_form(c, host_counts) : and_batch_rounds(c, searched0, host_counts);
    }
    if (st != DINT_OK) return st;
    HIP_TRY(hipGetLastError());
    if (extra) {
        st = bool_exclude_pass(c);
        if (st != DINT_OK) return st;
    }
    if (freqs_dict) {
        st = and_freqs_pass(c);
        if (st != DINT_OK) return st;
    }
    return and_copy_back(c, freq_sums, freq_blocks);
}

int dint_and_queries(dint_query_index* qi, const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries,
                     uint64_t* counts, void* stream) {
    return and_queries_impl(qi, nullptr, terms, query_offsets, n_queries, counts, nullptr, nullptr, stream, ranked_extras());
}

int dint_and_queries_freqs(dint_query_index* qi, const dint_dict* freqs_dict, const uint32_t* terms, const uint64_t* query_offsets,
                           size_t n_queries, uint64_t* counts, uint64_t* freq_sums, uint64_t* freq_blocks_decoded, void* stream) {
    if (!freqs_args_ok(qi, freqs_dict, freq_sums)) return DINT_ERR_ARG;
    return and_queries_impl(qi, freqs_dict, terms, query_offsets, n_queries, counts, freq_sums, freq_blocks_decoded, stream, ranked_extras());
}
