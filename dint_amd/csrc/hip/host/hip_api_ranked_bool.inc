// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": ranked boolean queries — required,
// optional and excluded terms (ranked_and_query, queries.hpp:309-385, generalised; next_geq + freq(),
// dict_posting_list.hpp:126-169: DESIGN.md 4d-bool).
// ---- ranked boolean queries -----------------------------------------------------------------------
// A ranked boolean call is a ranked AND call over the required terms (and_queries_impl with rk) with extra steps
// (bool_steps) hooked into it:
//   1 the AND rounds leave the survivors in their candidate slots
//   2 per excluded term, in ascending term id: search -> claim -> the claimed blocks' docs parts decoded -> a candidate
//     found is killed -> release (bool_exclude_pass), then
//   3 the matches are counted again
//   4 the required terms are scored by and_freqs_pass's own loop
//   5 per optional term, in ascending term id: search -> claim -> the claimed blocks' docs and freqs parts decoded -> a
//     match found adds its addend -> release (bool_should_pass)
//   6 ranked_topk, 7 the copy back
// Step j of a clause serves the j-th term of every query that has one, like a round of the AND path. A step claims at most
// min(sum over the queries of the term's blocks, candidate slots) blocks: the launches are sized for that bound and the
// pages past the claimed ones are empty; past kAsyncPages the count is read back, as in the freqs pass.

// the tables into the staging area, behind the general form's; where the kernels read them
static void bool_stage_steps(and_call& c, const and_bool_layout& L) {
    dint_query_index* qi = c.qi;
    bool_steps& x = *c.extra;
    std::memcpy(qi->h(L.not_first), x.not_first.data(), x.not_first.size() * 4);
    std::memcpy(qi->h(L.not_blocks), x.not_blocks.data(), x.not_blocks.size() * 4);
    std::memcpy(qi->h(L.should_first), x.should_first.data(), x.should_first.size() * 4);
    std::memcpy(qi->h(L.should_blocks), x.should_blocks.data(), x.should_blocks.size() * 4);
    std::memcpy(qi->h<float>(L.should_weight), x.should_weight.data(), x.should_weight.size() * 4);
    std::memset(qi->h(L.step_count), 0, (x.n_not + x.n_should) * 4);
    x.d_not_first = qi->d(L.not_first);
    x.d_not_blocks = qi->d(L.not_blocks);
    x.d_should_first = qi->d(L.should_first);
    x.d_should_blocks = qi->d(L.should_blocks);
    x.d_should_weight = qi->d<const float>(L.should_weight);
    x.d_step_count = qi->d(L.step_count);
}

// One step over the slots `b`: `first` / `nblk` (device) and `h_nblk` (host) are the step's row of its clause's tables;
// weight null: an excluded term (docs parts only), else an optional one. The claims are the first set's, as in the freqs pass.
static int bool_step(const bool_slots& b, const uint32_t* first, const uint32_t* nblk, const uint32_t* h_nblk, const float* weight,
                     uint32_t* d_cnt) {
    dint_query_index* qi = b.qi;
    const uint32_t tb = 256;
    uint64_t list_blocks = 0;
    for (size_t q = 0; q != b.n_queries; ++q) list_blocks += h_nblk[q];
    size_t bound = size_t(std::min<uint64_t>(b.n_slots, list_blocks));
    if (bound == 0) return DINT_OK;
    hipLaunchKernelGGL(bool_search_kernel, dim3(b.slot_grid()), dim3(tb), 0, b.s, qi->cand.p, b.n_slots, b.d_page_query, first, nblk,
                       qi->d_block_max, qi->target.p, qi->d_needed, qi->d_rank, qi->d_touched, d_cnt);
    const uint32_t* d_count = d_cnt;
    const bool sized = weight ? sized_by_bound(bound, {{&qi->probe, bound * kPageSlots}, {&qi->fprobe, bound * kPageSlots}})
                              : sized_by_bound(bound, {{&qi->probe, bound * kPageSlots}});
    if (!sized) {
        uint32_t n_touched = 0;
        HIP_TRY(hipMemcpyAsync(&n_touched, d_cnt, 4, hipMemcpyDeviceToHost, b.s));
        HIP_TRY(hipStreamSynchronize(b.s));
        if (n_touched == 0) return DINT_OK;
        bound = n_touched;
        d_count = nullptr;
    }
    if (!qi->sub.ensure(bound) || !qi->probe.ensure(uint64_t(bound) * kPageSlots) || (weight && !qi->fprobe.ensure(uint64_t(bound) * kPageSlots)))
        return stream_failed(b.s, DINT_ERR_HIP);
    const int st = gather_decode_pages(qi, qi->d_touched, d_count, bound, 0, weight ? b.freqs_dict : nullptr, b.s);
    if (st != DINT_OK) return stream_failed(b.s, st);
    if (weight)
        hipLaunchKernelGGL(bool_should_gather_kernel, dim3(b.slot_grid()), dim3(tb), 0, b.s, qi->cand.p, b.n_slots, b.d_page_query, qi->d_blocks,
                           qi->target.p, qi->d_rank, qi->probe.p, qi->fprobe.p, weight, qi->slot_kden.p, qi->slot_score.p);
    else
        hipLaunchKernelGGL(bool_exclude_kernel, dim3(b.slot_grid()), dim3(tb), 0, b.s, qi->cand.p, b.n_slots, qi->d_blocks, qi->target.p,
                           qi->d_rank, qi->probe.p);
    hipLaunchKernelGGL(and_release_kernel, dim3(uint32_t((bound + tb - 1) / tb)), dim3(tb), 0, b.s, qi->d_touched, uint32_t(bound), qi->d_needed,
                       d_count);
    return DINT_OK;
}
// the slots of an AND call: its candidates
static bool_slots bool_slots_of(const and_call& c) { return {c.qi, c.freqs_dict, c.n_slots, c.d_page_query, c.n_queries, c.s}; }

// Behind the AND rounds, before anything is scored: the excluded terms' steps, then the matches counted again (the rounds
// counted the intersection).
static int bool_exclude_pass(and_call& c) {
    const bool_steps& x = *c.extra;
    const size_t nq = c.n_queries;
    if (x.n_not == 0) return DINT_OK;
    for (size_t j = 0; j != x.n_not; ++j) {
        const int st = bool_step(bool_slots_of(c), x.d_not_first + j * nq, x.d_not_blocks + j * nq, x.not_blocks.data() + j * nq, nullptr, x.d_step_count + j);
        if (st != DINT_OK) return st;
    }
    HIP_TRY(hipMemsetAsync(c.d_counts, 0, nq * sizeof(unsigned long long), c.s));
    hipLaunchKernelGGL(and_count_kernel, dim3(c.slot_grid()), dim3(256), 0, c.s, c.qi->cand.p, c.n_slots, c.d_page_query, c.d_counts);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}

// Behind the freqs pass's required terms: the optional terms' steps; every step's claim count on its way back.
static int bool_should_pass(and_call& c) {
    bool_steps& x = *c.extra;
    const size_t nq = c.n_queries;
    for (size_t j = 0; j != x.n_should; ++j) {
        const int st = bool_step(bool_slots_of(c), x.d_should_first + j * nq, x.d_should_blocks + j * nq, x.should_blocks.data() + j * nq,
                                 x.d_should_weight + j * nq, x.d_step_count + x.n_not + j);
        if (st != DINT_OK) return st;
    }
    HIP_TRY(hipGetLastError());
    x.h_claims.assign(x.n_not + x.n_should, 0);
    if (!x.h_claims.empty())
        HIP_TRY(hipMemcpyAsync(x.h_claims.data(), x.d_step_count, x.h_claims.size() * 4, hipMemcpyDeviceToHost, c.s));
    return DINT_OK;
}

namespace {
// A clause as the caller gives it: null offsets (empty for every query), or offsets / terms as in every query call.
struct bool_clause {
    const uint32_t* terms;
    const uint64_t* offsets;
    bool ok(const dint_query_index* qi, size_t n_queries) const {
        if (!offsets) return true;
        for (size_t q = 0; q != n_queries; ++q)
            if (offsets[q + 1] < offsets[q]) return false;
        if (offsets[n_queries] != offsets[0] && !terms) return false;
        for (uint64_t i = offsets[0]; i != offsets[n_queries]; ++i)
            if (terms[i] >= qi->list_len.size()) return false;
        return true;
    }
    // query q's distinct terms in ascending term id, each with its multiplicity
    void of(size_t q, std::vector<std::pair<uint32_t, uint32_t>>& out) const {
        out.clear();
        if (!offsets) return;
        std::vector<uint32_t> t(terms + offsets[q], terms + offsets[q + 1]);
        std::sort(t.begin(), t.end());
        for (uint32_t v : t)
            if (!out.empty() && out.back().first == v) out.back().second += 1;
            else out.emplace_back(v, 1u);
    }
};
}  // namespace

int dint_ranked_bool_queries(dint_query_index* qi, const dint_dict* freqs_dict, const dint_wand_data* wd, uint32_t k,
                             const uint32_t* must_terms, const uint64_t* must_offsets, const uint32_t* should_terms,
                             const uint64_t* should_offsets, const uint32_t* not_terms, const uint64_t* not_offsets, size_t n_queries,
                             uint64_t* counts, uint64_t* matches, float* scores, uint32_t* docids, uint64_t* blocks_decoded, void* stream) {
    // (a null must clause selects nothing, but is checked like one of empty queries)
    const std::vector<uint64_t> no_offsets(must_offsets ? 0 : n_queries + 1, 0);
    if (!must_offsets) must_offsets = no_offsets.data();
    if (!ranked_args_ok(qi, freqs_dict, wd, k, must_offsets, n_queries, counts, scores)) return DINT_ERR_ARG;
    const bool_clause should{should_terms, should_offsets}, exclude{not_terms, not_offsets};
    if (!bool_clause{must_terms, must_offsets}.ok(qi, n_queries) || !should.ok(qi, n_queries) || !exclude.ok(qi, n_queries)) return DINT_ERR_ARG;
    if (blocks_decoded) *blocks_decoded = 0;
    if (n_queries == 0) return DINT_OK;

    // the step tables: a query without a required term selects nothing, and has no step
    bool_steps x;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> sh(n_queries), ex(n_queries);
    for (size_t q = 0; q != n_queries; ++q) {
        if (must_offsets[q + 1] == must_offsets[q]) continue;
        should.of(q, sh[q]);
        exclude.of(q, ex[q]);
        x.n_should = std::max(x.n_should, sh[q].size());
        x.n_not = std::max(x.n_not, ex[q].size());
    }
    x.not_first.assign(x.n_not * n_queries, 0);
    x.not_blocks.assign(x.n_not * n_queries, 0);
    x.should_first.assign(x.n_should * n_queries, 0);
    x.should_blocks.assign(x.n_should * n_queries, 0);
    x.should_weight.assign(x.n_should * n_queries, 0.0f);
    for (size_t q = 0; q != n_queries; ++q) {
        for (size_t j = 0; j != ex[q].size(); ++j) {
            x.not_first[j * n_queries + q] = qi->list_first[ex[q][j].first];
            x.not_blocks[j * n_queries + q] = qi->blocks_of(ex[q][j].first);
        }
        for (size_t j = 0; j != sh[q].size(); ++j) {
            const uint32_t t = sh[q][j].first;
            x.should_first[j * n_queries + q] = qi->list_first[t];
            x.should_blocks[j * n_queries + q] = qi->blocks_of(t);
            x.should_weight[j * n_queries + q] = bm25_query_term_weight(sh[q][j].second, qi->list_len[t], wd->num_docs);
        }
    }

    std::vector<unsigned long long> keys(uint64_t(n_queries) * k, 0ull);
    std::vector<uint64_t> freq_sums(n_queries, 0);
    const ranked_args rk = ranked_args_of(wd, k, keys.data());
    uint64_t must_claims = 0;
    const int st = and_queries_impl(qi, freqs_dict, must_terms, must_offsets, n_queries, counts, freq_sums.data(), &must_claims, stream,
                                    ranked_extras(), false, &rk, &x);
    if (st != DINT_OK) return st;
    if (blocks_decoded) {
        *blocks_decoded = must_claims;
        for (uint32_t n : x.h_claims) *blocks_decoded += n;
    }
    for (size_t q = 0; q != n_queries; ++q) {
        if (matches) matches[q] = counts[q];
        counts[q] = std::min<uint64_t>(counts[q], k);
    }
    unpack_keys(keys, n_queries, k, counts, scores, docids);
    return DINT_OK;
}
