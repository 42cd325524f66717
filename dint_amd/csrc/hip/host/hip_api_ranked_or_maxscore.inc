// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": MaxScore-pruned ranked
// disjunctive queries (the pruning of maxscore_query, queries.hpp:459-573, with ranked_or_query's sums: DESIGN.md 4d-maxscore).
// ---- pruned ranked disjunctive queries ----------------------------------------------------------
// The passes are an OR call's (plan_or_passes). Per pass:
//   seeds   per query, the shortest list of at least k postings (smaller term id on ties): its pages decoded with their
//           freqs, scored as one-term records by ranked_or_score_kernel, ranked_topk; theta = the k-th key's score, brought
//           back once (a query without a seed has theta 0 and prunes nothing)
//   split   on the host: N = the longest proper prefix of the terms by (m_t = q_weight_t * max_term_weight_t ascending, term
//           id) with (sum_N m_t) * margin < theta, E = the rest; margin = 1 + (|T| + 1) * 2^-23 (the reordering of the binary32
//           sum, DESIGN.md 4d-maxscore)
//   E       the other E terms' pages decoded behind the seeds'; ms_bound_kernel over E's pages (the seed's own reused); a wand
//           handle with block maxima (dint_wand_data_set_block_max_weights) bounds N per candidate, by the blocks it falls in
//   claims  the claimed blocks decoded behind those; ms_score_kernel; ranked_topk
// Pages of a pass: seeds + E + claimed <= every block of every term, the pass bound of ranked_or.

// One pass of the call: what its three stages share. A query's records are consecutive, longest list first.
struct maxscore_pass_state {
    dint_query_index* qi;
    const dint_dict* freqs_dict;
    const dint_wand_data* wd;
    const query_plan& plan;
    uint64_t* read;  // blocks read, per query of the call
    hipStream_t s;
    ranked_args rk;  // (keys: the pass's part of the call's)
    size_t q0, nq;
    uint64_t n_rec = 0;
    std::vector<float> qw{};                               // per record: q_weight
    std::vector<uint32_t> q_from{}, seed{}, seed_page{};   // per query: its first record, its seed (~0u: none) and the seed's first page
    std::vector<float> theta{};                            // per query
    uint32_t S = 0, R = 0, F = 0, C = 0;                   // seed pages, E pages beside the seeds', claim flags, candidate pages
    std::vector<uint32_t> claimed{}, is_e{}, t_page{};     // per record
    std::vector<double> rest{}, margin{};                  // per query
    std::vector<uint32_t> rest_blocks{};                   // the other E terms' blocks, in page order
};

// ---- seeds: theta. The q_weights and every query's seed; the seeds' pages as one-term records through the ranked OR
// pass (or_run_pass), the k-th key's score brought back with the one wait for theta ----
static int maxscore_seeds(maxscore_pass_state& m) {
    const dint_query_index* qi = m.qi;
    const uint32_t k = m.rk.k;
    m.qw.resize(m.n_rec);
    m.q_from.resize(m.nq);
    m.seed.assign(m.nq, ~0u);
    m.seed_page.assign(m.nq, 0);
    m.theta.assign(m.nq, 0.0f);
    std::vector<or_pass_query> seeds;
    for (size_t i = 0, r = 0; i != m.nq; ++i) {
        m.q_from[i] = uint32_t(r);
        const uint32_t* t = m.plan.of(m.q0 + i);
        uint32_t& sd = m.seed[i];
        for (uint32_t j = 0; j != m.plan.len[m.q0 + i]; ++j, ++r) {
            m.qw[r] = bm25_query_term_weight(m.plan.qf_of(m.q0 + i)[j], qi->list_len[t[j]], m.wd->num_docs);
            if (qi->list_len[t[j]] < k) continue;
            if (sd == ~0u || qi->list_len[t[j]] < qi->list_len[t[sd]] || (qi->list_len[t[j]] == qi->list_len[t[sd]] && t[j] < t[sd])) sd = j;
        }
        if (sd == ~0u) continue;
        m.seed_page[i] = m.S;
        m.S += qi->blocks_of(t[sd]);
        seeds.push_back({uint32_t(i), 1u, t + sd, m.plan.qf_of(m.q0 + i) + sd});
    }
    if (m.S == 0) return DINT_OK;  // (a query without a seed has theta 0 and prunes nothing)
    std::vector<unsigned long long> seed_keys(m.nq * k, 0ull);
    ranked_args seed_rk = m.rk;
    seed_rk.keys = seed_keys.data();
    const int st = or_run_pass(m.qi, m.freqs_dict, &seed_rk, seeds, /*min_stage*/ 0, /*no counters*/ nullptr, 0, /*ids*/ 0u, m.nq, m.s,
                               ranked_extras());
    if (st != DINT_OK) return st;
    HIP_TRY(hipStreamSynchronize(m.s));  // (the one wait for theta)
    for (size_t i = 0; i != m.nq; ++i) {
        const uint32_t bits = uint32_t(seed_keys[i * k + k - 1] >> 32);
        std::memcpy(&m.theta[i], &bits, 4);
    }
    return DINT_OK;
}

// ---- the split, and the layout of the pages: seeds [0, S), the other E terms [S, S + R), claims [S + R, ...) ----
static void maxscore_split(maxscore_pass_state& m) {
    const dint_query_index* qi = m.qi;
    m.claimed.assign(m.n_rec, 0);
    m.is_e.assign(m.n_rec, 0);
    m.t_page.assign(m.n_rec, 0);
    m.rest.assign(m.nq, 0.0);
    m.margin.assign(m.nq, 1.0);
    std::vector<uint32_t> ord;
    std::vector<float> mw;
    for (size_t i = 0; i != m.nq; ++i) {
        const size_t q = m.q0 + i;
        const uint32_t n = m.plan.len[q], from = m.q_from[i];
        const uint32_t* t = m.plan.of(q);
        m.margin[i] = 1.0 + double(n + 1) * 0x1p-23;
        uint32_t n_n = 0;  // |N|
        if (m.theta[i] > 0.0f) {
            mw.resize(n);
            for (uint32_t j = 0; j != n; ++j) mw[j] = m.qw[from + j] * m.wd->max_term_weight[t[j]];
            ord.resize(n);
            for (uint32_t j = 0; j != n; ++j) ord[j] = j;
            std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return mw[a] != mw[b] ? mw[a] < mw[b] : t[a] < t[b]; });
            double sum = 0.0;
            for (; n_n + 1 < n; ++n_n) {  // (E is never empty)
                const double next = sum + double(mw[ord[n_n]]);
                if (!(next * m.margin[i] < double(m.theta[i]))) break;
                sum = next;
            }
            m.rest[i] = sum;
            for (uint32_t x = n_n; x != n; ++x) m.is_e[from + ord[x]] = 1;
        } else {
            for (uint32_t j = 0; j != n; ++j) m.is_e[from + j] = 1;
        }
        for (uint32_t j = 0; j != n; ++j) {
            const uint32_t r = from + j, nb = qi->blocks_of(t[j]);
            if (j == m.seed[i]) {
                m.t_page[r] = m.seed_page[i];
                m.read[q] += nb;
                if (!m.is_e[r]) m.claimed[r] = 2;  // (a seed in N: decoded, but bounded like any N term under block maxima)
            } else if (m.is_e[r]) {
                m.t_page[r] = m.S + m.R;
                for (uint32_t b = 0; b != nb; ++b) m.rest_blocks.push_back(qi->list_first[t[j]] + b);
                m.R += nb;
                m.read[q] += nb;
            } else {
                m.claimed[r] = 1;
                m.t_page[r] = m.F;
                m.F += nb;
            }
            if (m.is_e[r]) m.C += nb;
        }
    }
}

// ---- E, claims, scores: the inputs (maxscore_layout) in; the other E terms' pages decoded behind the seeds';
// ms_bound_kernel over E's pages; the claimed blocks decoded behind those (sized for every block the N terms have; the
// pages past the claimed ones are empty); ms_score_kernel; ranked_topk; the keys and the claims back with one wait ----
static int maxscore_main(maxscore_pass_state& m) {
    dint_query_index* qi = m.qi;
    const size_t nq = m.nq;
    const uint32_t S = m.S, R = m.R, F = m.F, C = m.C;
    const maxscore_layout L(m.n_rec, nq, C, R);
    if (qi->stage(L.words * 4) != hipSuccess) return stream_failed(m.s, DINT_ERR_HIP);
    uint32_t *h_blocks = qi->h(L.term_blocks), *h_order = qi->h(L.term_order), *h_e = qi->h(L.term_e), *h_cpage = qi->h(L.cpage_page),
             *h_crec = qi->h(L.cpage_rec);
    std::vector<uint32_t> cpage_query(C);  // (ranked_topk's)
    uint32_t cp = 0;
    for (size_t i = 0; i != nq; ++i) {
        const uint32_t n = m.plan.len[m.q0 + i], from = m.q_from[i];
        const uint32_t* t = m.plan.of(m.q0 + i);
        uint32_t ne = 0;
        for (uint32_t j = 0; j != n; ++j) {
            const uint32_t r = from + j;
            qi->h(L.term_first)[r] = qi->list_first[t[j]];
            h_blocks[r] = qi->blocks_of(t[j]);
            qi->h(L.term_page)[r] = m.t_page[r];
            qi->h(L.term_claimed)[r] = m.claimed[r];
            qi->h<float>(L.term_weight)[r] = m.qw[r];
            qi->h(L.rec_query)[r] = uint32_t(i);
            if (!m.is_e[r]) continue;
            h_e[from + ne++] = r;
            for (uint32_t b = 0; b != h_blocks[r]; ++b, ++cp) {
                h_cpage[cp] = m.t_page[r] + b;
                h_crec[cp] = r;
                cpage_query[cp] = uint32_t(i);
            }
        }
        sort_records_by_term(h_order, from, n, t);
        qi->h(L.q_from)[i] = from;
        qi->h(L.q_n)[i] = n;
        qi->h(L.q_ne)[i] = ne;
        qi->h<float>(L.q_theta)[i] = m.theta[i];
        qi->h<double>(L.q_rest)[i] = m.rest[i];
        qi->h<double>(L.q_margin)[i] = m.margin[i];
    }
    std::copy(m.rest_blocks.begin(), m.rest_blocks.end(), qi->h(L.rest_blocks));
    if (!qi->inputs.ensure(L.words) || !qi->ms_count.ensure(1 + nq) || !qi->ms_flag.ensure(std::max<uint32_t>(1, F)) ||
        !qi->ms_rank.ensure(std::max<uint32_t>(1, F)) || !qi->ms_touched.ensure(std::max<uint32_t>(1, F)))
        return stream_failed(m.s, DINT_ERR_HIP);
    HIP_TRY(hipMemcpyAsync(qi->inputs.p, qi->h_stage, L.words * 4, hipMemcpyHostToDevice, m.s));
    HIP_TRY(hipMemsetAsync(qi->ms_count.p, 0, (1 + nq) * 4, m.s));
    if (F) HIP_TRY(hipMemsetAsync(qi->ms_flag.p, 0, size_t(F) * 4, m.s));
    if (R) {
        const int st = gather_decode_pages(qi, qi->d(L.rest_blocks), nullptr, R, S, m.freqs_dict, m.s);
        if (st != DINT_OK) return stream_failed(m.s, st);
    }
    maxscore_pass mp{};
    mp.term_first = qi->d(L.term_first);
    mp.term_blocks = qi->d(L.term_blocks);
    mp.term_page = qi->d(L.term_page);
    mp.term_claimed = qi->d(L.term_claimed);
    mp.term_weight = qi->d<const float>(L.term_weight);
    mp.term_order = qi->d(L.term_order);
    mp.term_e = qi->d(L.term_e);
    mp.rec_query = qi->d(L.rec_query);
    mp.q_from = qi->d(L.q_from);
    mp.q_n = qi->d(L.q_n);
    mp.q_ne = qi->d(L.q_ne);
    mp.q_theta = qi->d<const float>(L.q_theta);
    mp.cpage_page = qi->d(L.cpage_page);
    mp.cpage_rec = qi->d(L.cpage_rec);
    mp.q_rest = qi->d<const double>(L.q_rest);
    mp.q_margin = qi->d<const double>(L.q_margin);
    mp.blocks = qi->d_blocks;
    mp.block_max = qi->d_block_max;
    mp.docs = qi->probe.p;
    mp.freqs = qi->fprobe.p;
    mp.claim_page0 = S + R;
    mp.flag = qi->ms_flag.p;
    mp.rank = qi->ms_rank.p;
    mp.touched = qi->ms_touched.p;
    mp.n_touched = qi->ms_count.p;
    mp.q_claims = qi->ms_count.p + 1;
    mp.norm_lens = m.wd->d_norm_lens;
    mp.block_max_weight = m.wd->has_block_max ? m.wd->d_block_max_weight : nullptr;
    mp.cand = qi->cand.p;
    mp.score = qi->slot_score.p;
    hipLaunchKernelGGL(ms_bound_kernel, dim3(C), dim3(kPageSlots), 0, m.s, mp);
    if (F) {
        const int st = gather_decode_pages(qi, qi->ms_touched.p, qi->ms_count.p, F, uint64_t(S) + R, m.freqs_dict, m.s);
        if (st != DINT_OK) return stream_failed(m.s, st);
    }
    hipLaunchKernelGGL(ms_score_kernel, dim3(C), dim3(kPageSlots), 0, m.s, mp);
    if (hipGetLastError() != hipSuccess) return stream_failed(m.s, DINT_ERR_HIP);
    const int rst = ranked_topk(qi, m.rk, cpage_query, nq, m.s);
    if (rst != DINT_OK) return stream_failed(m.s, rst);
    std::vector<uint32_t> q_claims(nq, 0);
    HIP_TRY(hipMemcpyAsync(q_claims.data(), qi->ms_count.p + 1, nq * 4, hipMemcpyDeviceToHost, m.s));
    HIP_TRY(hipStreamSynchronize(m.s));  // (the staging area is free for the next pass; the keys and claims are here)
    for (size_t i = 0; i != nq; ++i) m.read[m.q0 + i] += q_claims[i];
    return DINT_OK;
}

int dint_ranked_or_maxscore_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts,
                                    float* scores, uint32_t* docids, uint64_t* blocks_read, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    if (!wd->has_max_weights || wd->max_term_weight.size() < qi->list_len.size()) return DINT_ERR_ARG;
    if (wd->has_block_max && wd->n_block_max != qi->n_blocks) return DINT_ERR_ARG;
    if (blocks_read) *blocks_read = 0;
    if (n_queries == 0) return DINT_OK;
    or_passes op;
    const int planned = plan_or_passes(qi, terms, query_offsets, n_queries, true, true, counts, nullptr, op);
    if (planned != DINT_OK) return planned;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    std::vector<uint64_t> read(n_queries, 0);  // blocks read per query
    if (op.all != 0) {
        std::lock_guard<std::mutex> lock(qi->mutex);
        HIP_TRY(hipSetDevice(qi->docs->device));
        hipStream_t s = static_cast<hipStream_t>(stream);
        for (size_t pass = 0; pass + 1 < op.first.size(); ++pass) {
            const size_t q0 = op.first[pass], q1 = op.first[pass + 1];
            maxscore_pass_state m{qi, freqs_dict, wd, op.plan, read.data(), s, ranked_args_of(wd, k, keys.data() + uint64_t(q0) * k), q0, q1 - q0};
            uint64_t n_pages = 0;
            for (size_t q = q0; q != q1; ++q) {
                n_pages += op.pages[q];
                m.n_rec += op.plan.len[q];
            }
            if (n_pages == 0) continue;
            if (!qi->sub.ensure(n_pages) || !qi->probe.ensure(n_pages * kPageSlots) || !qi->fprobe.ensure(n_pages * kPageSlots) ||
                !qi->cand.ensure(n_pages * kPageSlots) || !qi->slot_score.ensure(n_pages * kPageSlots))
                return stream_failed(s, DINT_ERR_HIP);
            int st = maxscore_seeds(m);
            if (st != DINT_OK) return st;
            maxscore_split(m);
            if (m.C == 0) continue;  // (no E term has a block: nothing to select; the keys stay 0)
            st = maxscore_main(m);
            if (st != DINT_OK) return st;
        }
    }
    counts_from_keys(keys, n_queries, k, counts);
    if (blocks_read)
        for (size_t q = 0; q != n_queries; ++q) *blocks_read += read[q];
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
