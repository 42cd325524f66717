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
//   E       the other E terms' pages decoded behind the seeds'; ms_bound_kernel over E's pages (the seed's own reused)
//   claims  the claimed blocks decoded behind those; ms_score_kernel; ranked_topk
// Pages of a pass: seeds + E + claimed <= every block of every term, the pass bound of ranked_or.

int dint_ranked_or_maxscore_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                                    const uint32_t* terms, const uint64_t* query_offsets, size_t n_queries, uint64_t* counts,
                                    float* scores, uint32_t* docids, uint64_t* blocks_read, void* stream) {
    if (!ranked_args_ok(qi, freqs_dict, wd, k, query_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    if (!wd->has_max_weights || wd->max_term_weight.size() < qi->list_len.size()) return DINT_ERR_ARG;
    if (blocks_read) *blocks_read = 0;
    if (n_queries == 0) return DINT_OK;
    or_passes op;
    const int planned = plan_or_passes(qi, terms, query_offsets, n_queries, true, true, counts, nullptr, op);
    if (planned != DINT_OK) return planned;
    const query_plan& plan = op.plan;
    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    std::vector<uint64_t> read(n_queries, 0);  // blocks read per query
    auto list_blocks = [&](uint32_t l) { return qi->list_first[l + 1] - qi->list_first[l]; };
    if (op.all != 0) {
        std::lock_guard<std::mutex> lock(qi->mutex);
        HIP_TRY(hipSetDevice(qi->docs->device));
        hipStream_t s = static_cast<hipStream_t>(stream);
        auto failed = [&](int st) {
            (void)hipStreamSynchronize(s);
            return st;
        };
        ranked_args rk{};
        rk.norm_lens = wd->d_norm_lens;
        rk.k = k;
        rk.num_docs = wd->num_docs;
        const uint32_t tb = 256;
        for (size_t pass = 0; pass + 1 < op.first.size(); ++pass) {
            const size_t q0 = op.first[pass], q1 = op.first[pass + 1], nq = q1 - q0;
            uint64_t n_pages = 0, n_rec = 0;
            for (size_t q = q0; q != q1; ++q) {
                n_pages += op.pages[q];
                n_rec += plan.len[q];
            }
            if (n_pages == 0) continue;
            // per record (a query's terms consecutive, longest list first): q_weight; per query: its first record, its seed
            std::vector<float> qw(n_rec);
            std::vector<uint32_t> q_from(nq), seed(nq, ~0u), seed_page(nq, 0);
            uint32_t S = 0, n_seeds = 0;  // seed pages, seeds
            for (size_t q = q0, r = 0; q != q1; ++q) {
                q_from[q - q0] = uint32_t(r);
                const uint32_t* t = plan.of(q);
                for (uint32_t j = 0; j != plan.len[q]; ++j, ++r) {
                    qw[r] = bm25_query_term_weight(plan.qf_of(q)[j], qi->list_len[t[j]], wd->num_docs);
                    if (qi->list_len[t[j]] < k) continue;
                    uint32_t& sd = seed[q - q0];
                    if (sd == ~0u || qi->list_len[t[j]] < qi->list_len[t[sd]] ||
                        (qi->list_len[t[j]] == qi->list_len[t[sd]] && t[j] < t[sd]))
                        sd = j;
                }
                if (seed[q - q0] != ~0u) {
                    seed_page[q - q0] = S;
                    S += list_blocks(t[seed[q - q0]]);
                    n_seeds += 1;
                }
            }
            if (!qi->sub.ensure(n_pages) || !qi->probe.ensure(n_pages * kPageSlots) || !qi->fprobe.ensure(n_pages * kPageSlots) ||
                !qi->cand.ensure(n_pages * kPageSlots) || !qi->slot_score.ensure(n_pages * kPageSlots))
                return failed(DINT_ERR_HIP);
            // ---- seeds: theta ----
            std::vector<float> theta(nq, 0.0f);
            if (S != 0) {
                // page -> block, page -> seed record, per seed record {first block, blocks, first page, query, from, order, n, q_weight}
                const size_t words = 2 * size_t(S) + 8 * size_t(n_seeds);
                if (qi->stage(words * 4) != hipSuccess) return failed(DINT_ERR_HIP);
                uint32_t* const h = static_cast<uint32_t*>(qi->h_stage);
                uint32_t *page_block = h, *page_term = h + S, *r_first = h + 2 * S, *r_blocks = r_first + n_seeds,
                         *r_page = r_blocks + n_seeds, *r_query = r_page + n_seeds, *r_from = r_query + n_seeds,
                         *r_order = r_from + n_seeds, *r_n = r_order + n_seeds;
                float* const r_weight = reinterpret_cast<float*>(r_n + n_seeds);
                std::vector<uint32_t> page_query(S);
                uint32_t page = 0, rec = 0;
                for (size_t i = 0; i != nq; ++i) {
                    if (seed[i] == ~0u) continue;
                    const uint32_t l = plan.of(q0 + i)[seed[i]];
                    r_first[rec] = qi->list_first[l];
                    r_blocks[rec] = list_blocks(l);
                    r_page[rec] = page;
                    r_query[rec] = uint32_t(i);
                    r_from[rec] = rec;
                    r_order[rec] = rec;
                    r_n[rec] = 1;
                    r_weight[rec] = qw[q_from[i] + seed[i]];
                    for (uint32_t b = qi->list_first[l]; b != qi->list_first[l + 1]; ++b, ++page) {
                        page_block[page] = b;
                        page_term[page] = rec;
                        page_query[page] = uint32_t(i);
                    }
                    ++rec;
                }
                if (!qi->inputs.ensure(words)) return failed(DINT_ERR_HIP);
                uint32_t* const d_in = qi->inputs.p;
                HIP_TRY(hipMemcpyAsync(d_in, h, words * 4, hipMemcpyHostToDevice, s));
                hipLaunchKernelGGL(gather_pages_kernel, dim3((S + tb - 1) / tb), dim3(tb), 0, s, qi->d_blocks, d_in, uint64_t(S), qi->sub.p,
                                   static_cast<const uint32_t*>(nullptr));
                const int st = decode_pages(qi, S, qi->probe.p, freqs_dict, qi->fprobe.p, s);
                if (st != DINT_OK) return failed(st);
                ranked_or_pass rp{};
                rp.base.page_block = d_in;
                rp.base.page_term = d_in + S;
                rp.base.term_first = d_in + 2 * S;
                rp.base.term_blocks = rp.base.term_first + n_seeds;
                rp.base.term_page = rp.base.term_blocks + n_seeds;
                rp.base.term_query = rp.base.term_page + n_seeds;
                rp.base.term_from = rp.base.term_query + n_seeds;
                rp.base.blocks = qi->d_blocks;
                rp.base.block_max = qi->d_block_max;
                rp.base.docs = qi->probe.p;
                rp.base.freqs = qi->fprobe.p;
                rp.term_order = rp.base.term_from + n_seeds;
                rp.term_n = rp.term_order + n_seeds;
                rp.term_weight = reinterpret_cast<const float*>(rp.term_n + n_seeds);
                rp.norm_lens = wd->d_norm_lens;
                rp.cand = qi->cand.p;
                rp.score = qi->slot_score.p;
                hipLaunchKernelGGL(ranked_or_score_kernel, dim3(S), dim3(kPageSlots), 0, s, rp);
                if (hipGetLastError() != hipSuccess) return failed(DINT_ERR_HIP);
                std::vector<unsigned long long> seed_keys(nq * k, 0ull);
                ranked_args seed_rk = rk;
                seed_rk.keys = seed_keys.data();
                const int rst = ranked_topk(qi, seed_rk, page_query, nq, s);
                if (rst != DINT_OK) return failed(rst);
                HIP_TRY(hipStreamSynchronize(s));  // (the one wait for theta)
                for (size_t i = 0; i != nq; ++i) {
                    const uint32_t bits = uint32_t(seed_keys[i * k + k - 1] >> 32);
                    std::memcpy(&theta[i], &bits, 4);
                }
            }
            // ---- the split, and the layout of the pages: seeds [0, S), the other E terms [S, S + R), claims [S + R, ...) ----
            std::vector<uint32_t> claimed(n_rec, 0), is_e(n_rec, 0), t_page(n_rec, 0);
            std::vector<double> rest(nq, 0.0), margin(nq, 1.0);
            std::vector<uint32_t> rest_blocks;  // the other E terms' blocks, in page order
            uint32_t R = 0, F = 0, C = 0;       // E pages beside the seeds', claim flags, candidate pages
            std::vector<uint32_t> ord;
            for (size_t i = 0; i != nq; ++i) {
                const size_t q = q0 + i;
                const uint32_t n = plan.len[q], from = q_from[i];
                const uint32_t* t = plan.of(q);
                margin[i] = 1.0 + double(n + 1) * 0x1p-23;
                uint32_t n_n = 0;  // |N|
                if (theta[i] > 0.0f) {
                    std::vector<float> m(n);
                    for (uint32_t j = 0; j != n; ++j) m[j] = qw[from + j] * wd->max_term_weight[t[j]];
                    ord.resize(n);
                    for (uint32_t j = 0; j != n; ++j) ord[j] = j;
                    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return m[a] != m[b] ? m[a] < m[b] : t[a] < t[b]; });
                    double sum = 0.0;
                    for (; n_n + 1 < n; ++n_n) {  // (E is never empty)
                        const double next = sum + double(m[ord[n_n]]);
                        if (!(next * margin[i] < double(theta[i]))) break;
                        sum = next;
                    }
                    rest[i] = sum;
                    for (uint32_t x = n_n; x != n; ++x) is_e[from + ord[x]] = 1;
                } else {
                    for (uint32_t j = 0; j != n; ++j) is_e[from + j] = 1;
                }
                for (uint32_t j = 0; j != n; ++j) {
                    const uint32_t r = from + j, nb = list_blocks(t[j]);
                    if (j == seed[i]) {
                        t_page[r] = seed_page[i];
                        read[q] += nb;
                    } else if (is_e[r]) {
                        t_page[r] = S + R;
                        for (uint32_t b = 0; b != nb; ++b) rest_blocks.push_back(qi->list_first[t[j]] + b);
                        R += nb;
                        read[q] += nb;
                    } else {
                        claimed[r] = 1;
                        t_page[r] = F;
                        F += nb;
                    }
                    if (is_e[r]) C += nb;
                }
            }
            if (C == 0) continue;  // (no E term has a block: nothing to select; the keys stay 0)
            // inputs: per record {first, blocks, page, claimed, q_weight, order, E, query}, per query {from, n, n_E, theta},
            // per candidate page {page, record}, the other E terms' blocks, then (8-byte aligned) per query {rest, margin}
            const size_t w_rec = 8 * n_rec, w_q = 4 * nq, dbl_at = (w_rec + w_q + 2 * size_t(C) + R + 1) / 2 * 2;
            const size_t words = dbl_at + 4 * nq;
            if (qi->stage(words * 4) != hipSuccess) return failed(DINT_ERR_HIP);
            uint32_t* const h = static_cast<uint32_t*>(qi->h_stage);
            uint32_t *h_first = h, *h_blocks = h + n_rec, *h_page = h_blocks + n_rec, *h_claimed = h_page + n_rec,
                     *h_order = h_claimed + 2 * n_rec, *h_e = h_order + n_rec, *h_rq = h_e + n_rec;
            float* const h_weight = reinterpret_cast<float*>(h_claimed + n_rec);
            uint32_t *h_qfrom = h + w_rec, *h_qn = h_qfrom + nq, *h_qne = h_qn + nq;
            float* const h_theta = reinterpret_cast<float*>(h_qne + nq);
            uint32_t *h_cpage = h + w_rec + w_q, *h_crec = h_cpage + C, *h_rest_blocks = h_crec + C;
            double* const h_dbl = reinterpret_cast<double*>(h + dbl_at);
            uint32_t cp = 0;
            for (size_t i = 0; i != nq; ++i) {
                const size_t q = q0 + i;
                const uint32_t n = plan.len[q], from = q_from[i];
                const uint32_t* t = plan.of(q);
                uint32_t ne = 0;
                for (uint32_t j = 0; j != n; ++j) {
                    const uint32_t r = from + j;
                    h_first[r] = qi->list_first[t[j]];
                    h_blocks[r] = list_blocks(t[j]);
                    h_page[r] = t_page[r];
                    h_claimed[r] = claimed[r];
                    h_weight[r] = qw[r];
                    h_order[r] = r;
                    h_rq[r] = uint32_t(i);
                    if (!is_e[r]) continue;
                    h_e[from + ne++] = r;
                    for (uint32_t b = 0; b != h_blocks[r]; ++b, ++cp) {
                        h_cpage[cp] = t_page[r] + b;
                        h_crec[cp] = r;
                    }
                }
                std::sort(h_order + from, h_order + from + n, [&](uint32_t a, uint32_t b) { return t[a - from] < t[b - from]; });
                h_qfrom[i] = from;
                h_qn[i] = n;
                h_qne[i] = ne;
                h_theta[i] = theta[i];
                h_dbl[i] = rest[i];
                h_dbl[nq + i] = margin[i];
            }
            std::copy(rest_blocks.begin(), rest_blocks.end(), h_rest_blocks);
            if (!qi->inputs.ensure(words) || !qi->ms_count.ensure(1 + nq) || !qi->ms_flag.ensure(std::max<uint32_t>(1, F)) ||
                !qi->ms_rank.ensure(std::max<uint32_t>(1, F)) || !qi->ms_touched.ensure(std::max<uint32_t>(1, F)))
                return failed(DINT_ERR_HIP);
            uint32_t* const d_in = qi->inputs.p;
            HIP_TRY(hipMemcpyAsync(d_in, h, words * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemsetAsync(qi->ms_count.p, 0, (1 + nq) * 4, s));
            if (F) HIP_TRY(hipMemsetAsync(qi->ms_flag.p, 0, size_t(F) * 4, s));
            if (R) {
                hipLaunchKernelGGL(gather_pages_kernel, dim3((R + tb - 1) / tb), dim3(tb), 0, s, qi->d_blocks, d_in + (h_rest_blocks - h),
                                   uint64_t(R), qi->sub.p, static_cast<const uint32_t*>(nullptr));
                const int st = decode_pages(qi, R, qi->probe.p + uint64_t(S) * kPageSlots, freqs_dict, qi->fprobe.p + uint64_t(S) * kPageSlots, s);
                if (st != DINT_OK) return failed(st);
            }
            maxscore_pass mp{};
            mp.term_first = d_in;
            mp.term_blocks = d_in + n_rec;
            mp.term_page = d_in + 2 * n_rec;
            mp.term_claimed = d_in + 3 * n_rec;
            mp.term_weight = reinterpret_cast<const float*>(d_in + 4 * n_rec);
            mp.term_order = d_in + 5 * n_rec;
            mp.term_e = d_in + 6 * n_rec;
            mp.rec_query = d_in + 7 * n_rec;
            mp.q_from = d_in + w_rec;
            mp.q_n = mp.q_from + nq;
            mp.q_ne = mp.q_n + nq;
            mp.q_theta = reinterpret_cast<const float*>(mp.q_ne + nq);
            mp.cpage_page = d_in + w_rec + w_q;
            mp.cpage_rec = mp.cpage_page + C;
            mp.q_rest = reinterpret_cast<const double*>(d_in + dbl_at);
            mp.q_margin = mp.q_rest + nq;
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
            mp.norm_lens = wd->d_norm_lens;
            mp.cand = qi->cand.p;
            mp.score = qi->slot_score.p;
            hipLaunchKernelGGL(ms_bound_kernel, dim3(C), dim3(kPageSlots), 0, s, mp);
            if (F) {  // (sized for every block the N terms have; the pages past the claimed ones are empty)
                hipLaunchKernelGGL(gather_pages_kernel, dim3((F + tb - 1) / tb), dim3(tb), 0, s, qi->d_blocks, qi->ms_touched.p, uint64_t(F),
                                   qi->sub.p, static_cast<const uint32_t*>(qi->ms_count.p));
                const uint64_t at = uint64_t(S + R) * kPageSlots;
                const int st = decode_pages(qi, F, qi->probe.p + at, freqs_dict, qi->fprobe.p + at, s);
                if (st != DINT_OK) return failed(st);
            }
            hipLaunchKernelGGL(ms_score_kernel, dim3(C), dim3(kPageSlots), 0, s, mp);
            if (hipGetLastError() != hipSuccess) return failed(DINT_ERR_HIP);
            std::vector<uint32_t> cpage_query(C);
            for (uint32_t c = 0; c != C; ++c) cpage_query[c] = h_rq[h_crec[c]];
            ranked_args pass_rk = rk;
            pass_rk.keys = keys.data() + uint64_t(q0) * k;
            const int rst = ranked_topk(qi, pass_rk, cpage_query, nq, s);
            if (rst != DINT_OK) return failed(rst);
            std::vector<uint32_t> q_claims(nq, 0);
            HIP_TRY(hipMemcpyAsync(q_claims.data(), qi->ms_count.p + 1, nq * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));  // (the staging area is free for the next pass; the keys and claims are here)
            for (size_t i = 0; i != nq; ++i) read[q0 + i] += q_claims[i];
        }
    }
    for (size_t q = 0; q != n_queries; ++q) {
        uint64_t c = 0;  // (every score is > 0, as for dint_ranked_or_queries)
        while (c != k && keys[q * k + c] != 0) ++c;
        counts[q] = c;
        if (blocks_read) *blocks_read += read[q];
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
