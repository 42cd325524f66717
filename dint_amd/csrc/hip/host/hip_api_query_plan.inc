// Part of dint_hip.hip (one translation unit; included from there, in order): what the query calls plan before they take the lock.
// ---- query planning -----------------------------------------------------------------------------

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
// (sv, a sorted call's sort_args below: stage 1 of the selection orders by the column's value instead of the score)
struct sort_args;
static int ranked_topk(dint_query_index* qi, const ranked_args& rk, const std::vector<uint32_t>& page_query, size_t n_queries,
                       hipStream_t s, const sort_args* sv = nullptr);

// A ranged call (hip_api_ranked_range.inc): every query's docID range, and what the call reports besides its answer. Where
// a call takes a null one there is no range: nothing is planned or launched differently.
struct range_args {
    const dint_doc_range* ranges = nullptr;     // per query of the call: [lo, hi)
    uint64_t blocks = 0;                        // out: the pages the call planned (OR: every term's blocks in range; AND: the rarest's)
    std::vector<unsigned long long> h_matches;  // out (OR): per query the union's documents in range
};
// The blocks of list l that can hold a docID of *r, as positions in the list (list_blocks_in_range over the handle's own
// copy of the block maxima); r null: every block.
static block_span blocks_in_range(const dint_query_index* qi, uint32_t l, const dint_doc_range* r) {
    const uint32_t nb = qi->blocks_of(l);
    if (!r) return {0, nb};
    return list_blocks_in_range(qi->block_max.data() + qi->list_first[l], nb, r->lo, r->hi);
}

// A document filter (dint_doc_filter_create, hip_api_doc_filter.inc): a bitmap over the docID space and, for the query
// index it was made for, which blocks are live under it. Immutable once created.
struct dint_doc_filter {
    const dint_query_index* qi = nullptr;  // the index whose block table live / live_before follow
    int device = 0;
    uint64_t num_docs = 0, n_set = 0, n_blocks = 0;
    uint64_t* d_bits = nullptr;             // ceil(num_docs / 64) words, masked at num_docs (at least one word)
    uint32_t* d_live_before = nullptr;      // n_blocks + 1
    std::vector<uint8_t> live;              // the host's copy of the flags: the filtered calls plan their pages here
    std::vector<uint32_t> live_before;      // ... and of d_live_before: a list's live blocks in O(1)
    doc_filter_view view() const { return doc_filter_view{d_bits, uint32_t(num_docs), d_live_before}; }
};
// A filtered call (hip_api_doc_filter.inc): its filter, and what the call reports besides its answer. Where a call takes a
// null one there is no filter: nothing is planned or launched differently.
struct filter_args {
    const dint_doc_filter* filter = nullptr;
    uint64_t blocks = 0;                        // out: the pages the call planned (OR: every term's live blocks; AND: the rarest's)
    std::vector<unsigned long long> h_matches;  // out (OR): per query the union's documents in the filter
};
// The pages a call plans for list l: its blocks in range (r null: every block), or under a filter its live blocks.
static uint32_t planned_blocks(const dint_query_index* qi, uint32_t l, const dint_doc_range* r, const filter_args* fl) {
    if (fl) return fl->filter->live_before[qi->list_first[l + 1]] - fl->filter->live_before[qi->list_first[l]];
    return blocks_in_range(qi, l, r).size();
}
// ... and whether block b (of the index) is one of them, for a b inside the list's span in range
static bool block_planned(const filter_args* fl, uint32_t b) { return !fl || fl->filter->live[b] != 0; }

// A facets handle (dint_doc_facets_create, hip_api_facets.inc): docID -> group, a word per document on the device, and the
// groups' sizes on the host. It belongs to a device, not to a query index. Immutable once created.
struct dint_doc_facets {
    int device = 0;
    uint64_t num_docs = 0, n_grouped = 0;
    uint32_t n_groups = 0;
    uint32_t* d_group_of = nullptr;  // max(1, num_docs) words
    std::vector<uint32_t> sizes;     // n_groups: the documents of every group
    doc_facets_view view() const { return doc_facets_view{d_group_of, uint32_t(num_docs), n_groups}; }
};
// A document-values handle (dint_doc_values_create, hip_api_doc_values.inc): docID -> value, a word per document on the
// device. Like the facets handle it belongs to a device, not to a query index. Immutable once created.
struct dint_doc_values {
    int device = 0;
    uint64_t num_docs = 0;
    uint32_t* d_values = nullptr;  // max(1, num_docs) words
    doc_values_view view() const { return doc_values_view{d_values, uint32_t(num_docs)}; }
};
// A faceted call (hip_api_facets.inc): the handle, the call's rows on the device — n_queries * n_groups counters in the
// query index's facet_rows workspace, cleared once per call, added to by every pass — and where they go on the host. Where a
// call takes a null one there are no facets: nothing is planned or launched differently.
struct facet_args {
    const dint_doc_facets* facets = nullptr;
    uint32_t* d_rows = nullptr;  // (set by facet_rows_clear)
    uint32_t* h_rows = nullptr;  // the caller's facet_counts (a collapsed call: null where the caller asks for no rows)
    size_t words(size_t n_queries) const { return n_queries * size_t(facets->n_groups); }
};
// the call is planned and has refused nothing: every row is zero until a pass says otherwise
static void facet_rows_begin(const facet_args* fa, size_t n_queries) {
    if (fa && fa->h_rows) std::fill(fa->h_rows, fa->h_rows + fa->words(n_queries), 0u);
}
// under the index's lock, once per call, in front of its first counting launch
static int facet_rows_clear(dint_query_index* qi, facet_args* fa, size_t n_queries, hipStream_t s) {
    if (!qi->facet_rows.ensure(fa->words(n_queries))) return DINT_ERR_HIP;
    fa->d_rows = qi->facet_rows.p;
    HIP_TRY(hipMemsetAsync(fa->d_rows, 0, fa->words(n_queries) * 4, s));
    return DINT_OK;
}
// facet_count_kernel over the n_pages pages of qi->cand; d_page_query[page] + q0: the page's query of the call
static int facet_count_launch(const dint_query_index* qi, const facet_args* fa, uint64_t n_pages, const uint32_t* d_page_query, uint32_t q0,
                              hipStream_t s) {
    hipLaunchKernelGGL(facet_count_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_pages * kPageSlots, d_page_query, q0,
                       fa->facets->view(), fa->d_rows);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the rows' way back, on the stream, in front of the call's last wait
static int facet_rows_back(const facet_args* fa, size_t n_queries, hipStream_t s) {
    if (!fa->h_rows) return DINT_OK;  // (a collapsed call that keeps its rows on the device)
    HIP_TRY(hipMemcpyAsync(fa->h_rows, fa->d_rows, fa->words(n_queries) * 4, hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A collapsed call (hip_api_collapse.inc): a faceted call — it needs fa, whose rows and staged page -> query table it
// reuses — that lets only the best document of every group into the selection. Its workspaces are the query index's, sized
// and cleared once per call (collapse_clear): the table of best keys, 8 bytes per (query, group), the survivors' counters,
// and the hits' groups and group matches, n_queries * k words each; per pass the slots' groups. Where a call takes a null
// one nothing is planned or launched differently.
struct collapse_args {
    uint32_t k = 0;
    uint32_t *h_hit_groups = nullptr, *h_hit_group_matches = nullptr;  // the caller's, n_queries * k each
    std::vector<unsigned long long> h_collapsed;                       // per query: the kept documents
    unsigned long long *d_best = nullptr, *d_collapsed = nullptr;      // (set by collapse_clear)
    uint32_t *d_hit_groups = nullptr, *d_hit_group_matches = nullptr;
};
// the call is planned and has refused nothing: no query has kept a document or has a hit until a pass says otherwise
static void collapse_begin(collapse_args* ca, size_t n_queries) {
    if (!ca) return;
    ca->h_collapsed.assign(n_queries, 0ull);
    std::fill(ca->h_hit_groups, ca->h_hit_groups + n_queries * ca->k, kFacetNone);
    std::fill(ca->h_hit_group_matches, ca->h_hit_group_matches + n_queries * ca->k, 0u);
}
// under the index's lock, once per call, in front of its first launch: the table (a live key is never 0) and the counters
// zero, every hit in no group with no matches
static int collapse_clear(dint_query_index* qi, collapse_args* ca, const facet_args* fa, size_t n_queries, hipStream_t s) {
    const size_t n_best = fa->words(n_queries), n_hits = n_queries * ca->k;
    if (!qi->collapse_best.ensure(n_best + n_queries) || !qi->collapse_hits.ensure(2 * n_hits)) return DINT_ERR_HIP;
    ca->d_best = qi->collapse_best.p;
    ca->d_collapsed = ca->d_best + n_best;
    ca->d_hit_groups = qi->collapse_hits.p;
    ca->d_hit_group_matches = ca->d_hit_groups + n_hits;
    HIP_TRY(hipMemsetAsync(ca->d_best, 0, (n_best + n_queries) * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(ca->d_hit_groups, 0xFF, n_hits * 4, s));
    HIP_TRY(hipMemsetAsync(ca->d_hit_group_matches, 0, n_hits * 4, s));
    return DINT_OK;
}
// collapse_best_kernel and collapse_keep_kernel over the n_pages pages of qi->cand, behind facet_count_launch (the rows
// count every match) and in front of ranked_topk; d_page_query[page] + q0: the page's query of the call
static int collapse_launch(dint_query_index* qi, const collapse_args* ca, const facet_args* fa, uint64_t n_pages,
                           const uint32_t* d_page_query, uint32_t q0, hipStream_t s) {
    const uint64_t n_slots = n_pages * kPageSlots;
    if (!qi->collapse_slot_group.ensure(n_slots)) return DINT_ERR_HIP;
    const doc_facets_view f = fa->facets->view();
    hipLaunchKernelGGL(collapse_best_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, qi->slot_score.p, n_slots,
                       d_page_query, q0, f, ca->d_best, qi->collapse_slot_group.p);
    hipLaunchKernelGGL(collapse_keep_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, qi->slot_score.p,
                       qi->collapse_slot_group.p, n_slots, d_page_query, q0, f.n_groups, ca->d_best, ca->d_collapsed);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// collapse_hits_kernel behind ranked_topk, over the keys it selected for the n_ids queries from q0 on (qi->topk_out)
static int collapse_hits_launch(const dint_query_index* qi, const collapse_args* ca, const facet_args* fa, size_t n_ids, uint32_t q0,
                                hipStream_t s) {
    const uint64_t n_out = uint64_t(n_ids) * ca->k;
    hipLaunchKernelGGL(collapse_hits_kernel, dim3(uint32_t((n_out + 255) / 256)), dim3(256), 0, s, qi->topk_out.p, uint32_t(n_ids), ca->k, q0,
                       fa->facets->view(), fa->d_rows, ca->d_hit_groups, ca->d_hit_group_matches);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the counters' and the hits' way back, on the stream, in front of the call's last wait
static int collapse_back(collapse_args* ca, size_t n_queries, hipStream_t s) {
    const size_t n_hits = n_queries * ca->k;
    HIP_TRY(hipMemcpyAsync(ca->h_collapsed.data(), ca->d_collapsed, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ca->h_hit_groups, ca->d_hit_groups, n_hits * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(ca->h_hit_group_matches, ca->d_hit_group_matches, n_hits * 4, hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A group-limited call (hip_api_group_limit.inc): a faceted call — it needs fa, whose rows and staged page -> query table it
// reuses, and is never combined with a collapse_args — that lets up to per_group documents of every group into the
// selection. Its workspaces are the query index's, sized and cleared once per call (group_limit_clear): the table of keys,
// 8 bytes per (query, place, group), the survivors' counters behind it, and the hits' groups, group matches and places,
// n_queries * k words each; per pass the slots' groups (collapse_slot_group). Where a call takes a null one nothing is
// planned or launched differently.
struct group_limit_args {
    uint32_t per_group = 0, k = 0;
    uint32_t *h_hit_groups = nullptr, *h_hit_group_matches = nullptr, *h_hit_group_ranks = nullptr;  // the caller's, n_queries * k each
    std::vector<unsigned long long> h_kept;                                                           // per query: the kept documents
    unsigned long long *d_top = nullptr, *d_kept = nullptr;                                           // (set by group_limit_clear)
    uint32_t *d_hit_groups = nullptr, *d_hit_group_matches = nullptr, *d_hit_group_ranks = nullptr;
};
// the call is planned and has refused nothing: no query has kept a document or has a hit until a pass says otherwise
static void group_limit_begin(group_limit_args* gl, size_t n_queries) {
    if (!gl) return;
    gl->h_kept.assign(n_queries, 0ull);
    std::fill(gl->h_hit_groups, gl->h_hit_groups + n_queries * gl->k, kFacetNone);
    std::fill(gl->h_hit_group_matches, gl->h_hit_group_matches + n_queries * gl->k, 0u);
    std::fill(gl->h_hit_group_ranks, gl->h_hit_group_ranks + n_queries * gl->k, 0u);
}
// under the index's lock, once per call, in front of its first launch: the table (a live key is never 0) and the counters
// zero, every hit in no group with no matches at place 0
static int group_limit_clear(dint_query_index* qi, group_limit_args* gl, const facet_args* fa, size_t n_queries, hipStream_t s) {
    const size_t n_top = fa->words(n_queries) * gl->per_group, n_hits = n_queries * gl->k;
    if (!qi->group_limit_top.ensure(n_top + n_queries) || !qi->group_limit_hits.ensure(3 * n_hits)) return DINT_ERR_HIP;
    gl->d_top = qi->group_limit_top.p;
    gl->d_kept = gl->d_top + n_top;
    gl->d_hit_groups = qi->group_limit_hits.p;
    gl->d_hit_group_matches = gl->d_hit_groups + n_hits;
    gl->d_hit_group_ranks = gl->d_hit_group_matches + n_hits;
    HIP_TRY(hipMemsetAsync(gl->d_top, 0, (n_top + n_queries) * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(gl->d_hit_groups, 0xFF, n_hits * 4, s));
    HIP_TRY(hipMemsetAsync(gl->d_hit_group_matches, 0, 2 * n_hits * 4, s));
    return DINT_OK;
}
// the rounds 0 .. per_group - 1 of group_limit_round_kernel, in stream order, and group_limit_keep_kernel over the n_pages
// pages of qi->cand, behind facet_count_launch (the rows count every match) and in front of page_after_kernel and
// ranked_topk; d_page_query[page] + q0: the page's query of the call
static int group_limit_launch(dint_query_index* qi, const group_limit_args* gl, const facet_args* fa, uint64_t n_pages,
                              const uint32_t* d_page_query, uint32_t q0, hipStream_t s) {
    const uint64_t n_slots = n_pages * kPageSlots;
    if (!qi->collapse_slot_group.ensure(n_slots)) return DINT_ERR_HIP;
    const doc_facets_view f = fa->facets->view();
    for (uint32_t r = 0; r != gl->per_group; ++r)
        hipLaunchKernelGGL(group_limit_round_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, qi->slot_score.p, n_slots,
                           d_page_query, q0, f, r, gl->per_group, gl->d_top, qi->collapse_slot_group.p);
    hipLaunchKernelGGL(group_limit_keep_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, qi->slot_score.p,
                       qi->collapse_slot_group.p, n_slots, d_page_query, q0, f.n_groups, gl->per_group, gl->d_top, gl->d_kept);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// group_limit_hits_kernel behind ranked_topk, over the keys it selected for the n_ids queries from q0 on (qi->topk_out)
static int group_limit_hits_launch(const dint_query_index* qi, const group_limit_args* gl, const facet_args* fa, size_t n_ids, uint32_t q0,
                                   hipStream_t s) {
    const uint64_t n_out = uint64_t(n_ids) * gl->k;
    hipLaunchKernelGGL(group_limit_hits_kernel, dim3(uint32_t((n_out + 255) / 256)), dim3(256), 0, s, qi->topk_out.p, uint32_t(n_ids), gl->k, q0,
                       fa->facets->view(), gl->per_group, fa->d_rows, gl->d_top, gl->d_hit_groups, gl->d_hit_group_matches,
                       gl->d_hit_group_ranks);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the counters' and the hits' way back, on the stream, in front of the call's last wait
static int group_limit_back(group_limit_args* gl, size_t n_queries, hipStream_t s) {
    const size_t n_hits = n_queries * gl->k;
    HIP_TRY(hipMemcpyAsync(gl->h_kept.data(), gl->d_kept, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(gl->h_hit_groups, gl->d_hit_groups, n_hits * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(gl->h_hit_group_matches, gl->d_hit_group_matches, n_hits * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(gl->h_hit_group_ranks, gl->d_hit_group_ranks, n_hits * 4, hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A paged call (hip_api_paging.inc): per query of the call a cursor key — the selection's key (collapse_key) of the last hit
// the caller has seen, kPageFromStart for a query read from the start, 0 where nothing lies after the cursor — and what the
// call reports besides its answer: per query the matches (a collapsed call: the kept documents) that are NOT after the
// cursor. The keys and the counters are a grow-only workspace of the query index, n_queries words each, uploaded and
// cleared once per call under the lock (page_begin_device); page_after_kernel runs directly in front of ranked_topk, behind
// the collapse launches where there are any. Where a call takes a null one nothing is planned or launched differently.
struct page_args {
    std::vector<unsigned long long> keys;       // per query: the cursor's key
    std::vector<unsigned long long> h_skipped;  // out: per query (a query the call did not run: 0)
    unsigned long long *d_keys = nullptr, *d_skipped = nullptr;  // (set by page_begin_device)
};
// the call is planned and has refused nothing: no query has skipped a match until a pass says otherwise
static void page_begin(page_args* pg, size_t n_queries) {
    if (pg) pg->h_skipped.assign(n_queries, 0ull);
}
// under the index's lock, once per call, in front of its first page_after_kernel launch: the keys go up, the counters clear
static int page_begin_device(dint_query_index* qi, page_args* pg, size_t n_queries, hipStream_t s) {
    if (!qi->page_keys.ensure(2 * n_queries)) return DINT_ERR_HIP;
    pg->d_keys = qi->page_keys.p;
    pg->d_skipped = pg->d_keys + n_queries;
    // (pageable host memory: the copy has left pg->keys when the call returns, and the call waits on the stream before it does)
    HIP_TRY(hipMemcpyAsync(pg->d_keys, pg->keys.data(), n_queries * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(pg->d_skipped, 0, n_queries * sizeof(unsigned long long), s));
    return DINT_OK;
}
// page_after_kernel over the n_pages pages of qi->cand, directly in front of ranked_topk; d_page_query[page] + q0: the
// page's query of the call
static int page_after_launch(const dint_query_index* qi, const page_args* pg, uint64_t n_pages, const uint32_t* d_page_query, uint32_t q0,
                             hipStream_t s) {
    hipLaunchKernelGGL(page_after_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, qi->slot_score.p, n_pages * kPageSlots,
                       d_page_query, q0, pg->d_keys, pg->d_skipped);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the counters' way back, on the stream, in front of the call's last wait
static int page_back(page_args* pg, size_t n_queries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(pg->h_skipped.data(), pg->d_skipped, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A sorted call (hip_api_doc_values.inc): the column and the order its hits come in, per query of the call the cursor's key
// K (dint_doc_values_kernels.hpp) and whether it has a cursor at all — every 64-bit pattern is a key, so the flag travels
// beside it — and what the call reports besides its answer: per query the matches NOT after the cursor, per (query, i) the
// BM25 score of hit i (a key has no room for it: sorted_hits_kernel recovers it behind the selection). The keys and the
// counters, the flags and the hit scores are two grow-only workspaces of the query index, sent and cleared once per call
// under the lock (sort_begin_device). Per OR pass / per AND call: scoring -> value_after_kernel -> ranked_topk by value ->
// sorted_hits_kernel. Where a call takes a null one nothing is planned or launched differently.
struct sort_args {
    const dint_doc_values* values = nullptr;
    uint32_t order = 0, k = 0;
    bool any_set = false;      // some query has a cursor: value_after_kernel runs
    bool want_scores = false;  // the caller takes the scores: sorted_hits_kernel runs
    std::vector<unsigned long long> keys;       // per query: the cursor's key
    std::vector<uint32_t> set;                  // per query: 0: from the start
    std::vector<unsigned long long> h_skipped;  // out: per query (a query the call did not run: 0)
    std::vector<float> h_hit_scores;            // out: n_queries * k (past a query's count: 0.0f)
    unsigned long long *d_keys = nullptr, *d_skipped = nullptr;  // (set by sort_begin_device)
    uint32_t* d_set = nullptr;
    float* d_hit_scores = nullptr;
};
// the call is planned and has refused nothing: no query has skipped a match or has a hit until a pass says otherwise
static void sort_begin(sort_args* sv, size_t n_queries) {
    if (!sv) return;
    sv->h_skipped.assign(n_queries, 0ull);
    sv->h_hit_scores.assign(n_queries * sv->k, 0.0f);
}
// under the index's lock, once per call, in front of its first launch: the keys and the flags go up, the counters and the
// hit scores clear
static int sort_begin_device(dint_query_index* qi, sort_args* sv, size_t n_queries, hipStream_t s) {
    const size_t n_hits = n_queries * sv->k;
    if (!qi->sort_keys.ensure(2 * n_queries) || !qi->sort_words.ensure(n_queries + n_hits)) return DINT_ERR_HIP;
    sv->d_keys = qi->sort_keys.p;
    sv->d_skipped = sv->d_keys + n_queries;
    sv->d_set = qi->sort_words.p;
    sv->d_hit_scores = reinterpret_cast<float*>(qi->sort_words.p + n_queries);
    // (pageable host memory: the copies have left sv when the call returns, and the call waits on the stream before it does)
    HIP_TRY(hipMemcpyAsync(sv->d_keys, sv->keys.data(), n_queries * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sv->d_set, sv->set.data(), n_queries * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(sv->d_skipped, 0, n_queries * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(sv->d_hit_scores, 0, n_hits * 4, s));
    return DINT_OK;
}
// value_after_kernel over the n_pages pages of qi->cand, directly in front of ranked_topk; d_page_query[page] + q0: the
// page's query of the call. A call without a cursor launches nothing.
static int value_after_launch(const dint_query_index* qi, const sort_args* sv, uint64_t n_pages, const uint32_t* d_page_query, uint32_t q0,
                              hipStream_t s) {
    if (!sv->any_set) return DINT_OK;
    hipLaunchKernelGGL(value_after_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_pages * kPageSlots, d_page_query, q0,
                       sv->values->view(), sv->order, sv->d_keys, sv->d_set, sv->d_skipped);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// sorted_hits_kernel behind ranked_topk, over the same pages and the keys it selected for the pass's queries (qi->topk_out)
static int sorted_hits_launch(const dint_query_index* qi, const sort_args* sv, uint64_t n_pages, const uint32_t* d_page_query, uint32_t q0,
                              hipStream_t s) {
    if (!sv->want_scores) return DINT_OK;
    hipLaunchKernelGGL(sorted_hits_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, qi->slot_score.p, n_pages * kPageSlots,
                       d_page_query, q0, sv->values->view(), sv->order, qi->topk_out.p, sv->k, sv->d_hit_scores);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the counters' and the hit scores' way back, on the stream, in front of the call's last wait
static int sort_back(sort_args* sv, size_t n_queries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(sv->h_skipped.data(), sv->d_skipped, n_queries * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    if (sv->want_scores)
        HIP_TRY(hipMemcpyAsync(sv->h_hit_scores.data(), sv->d_hit_scores, n_queries * sv->k * 4, hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A value-stats call (hip_api_value_stats.inc): the column and the bucket boundaries, where the call's records, rows and hit
// values go on the host, and where they live on the device — two grow-only workspaces of the query index: the records, 24
// bytes per query, and behind one another the edges, the rows (n_queries * (n_edges + 1) counters) and the hit values
// (n_queries * k words). The records go up as the empty record, the edges go up and the rest is cleared once per call under
// the lock (value_stats_clear), every pass adds, and everything comes back once. Where a call takes a null one nothing is
// planned or launched differently.
struct value_stats_args {
    const dint_doc_values* values = nullptr;
    const uint32_t* edges = nullptr;  // host, n_edges words, strictly ascending (checked by the entry)
    uint32_t n_edges = 0, k = 0;
    dint_value_stats* h_stats = nullptr;  // the caller's, n_queries
    uint32_t* h_rows = nullptr;           // the caller's bucket_counts (n_edges == 0: not touched)
    uint32_t* h_hit_values = nullptr;     // the caller's, n_queries * k, or null: hit_values_kernel does not run
    value_stats_rec* d_stats = nullptr;   // (set by value_stats_clear)
    uint32_t *d_edges = nullptr, *d_rows = nullptr, *d_hit_values = nullptr;
    size_t row_words(size_t n_queries) const { return n_edges ? n_queries * (size_t(n_edges) + 1) : 0; }
    size_t hit_words(size_t n_queries) const { return h_hit_values ? n_queries * k : 0; }
};
static_assert(sizeof(dint_value_stats) == sizeof(value_stats_rec) && offsetof(dint_value_stats, min) == offsetof(value_stats_rec, min),
              "the records travel as the caller's struct");
// the call is planned and has refused nothing: every record is empty, every row and hit value zero until a pass says otherwise
static void value_stats_begin(const value_stats_args* vs, size_t n_queries) {
    if (!vs) return;
    std::fill(vs->h_stats, vs->h_stats + n_queries, dint_value_stats{0, 0, 0xFFFFFFFFu, 0});
    if (vs->n_edges) std::fill(vs->h_rows, vs->h_rows + vs->row_words(n_queries), 0u);
    if (vs->h_hit_values) std::fill(vs->h_hit_values, vs->h_hit_values + vs->hit_words(n_queries), 0u);
}
// under the index's lock, once per call, in front of its first launch: the empty records (the caller's own, as
// value_stats_begin left them) and the edges go up, the rows and the hit values clear
static int value_stats_clear(dint_query_index* qi, value_stats_args* vs, size_t n_queries, hipStream_t s) {
    const size_t n_rows = vs->row_words(n_queries), n_hits = vs->hit_words(n_queries);
    if (!qi->value_stats_recs.ensure(3 * n_queries) || !qi->value_stats_words.ensure(vs->n_edges + n_rows + n_hits)) return DINT_ERR_HIP;
    vs->d_stats = reinterpret_cast<value_stats_rec*>(qi->value_stats_recs.p);
    vs->d_edges = qi->value_stats_words.p;
    vs->d_rows = vs->d_edges + vs->n_edges;
    vs->d_hit_values = vs->d_rows + n_rows;
    // (pageable host memory: the copies have left the caller's arrays when the call returns, and the call waits on the stream
    // before it does)
    HIP_TRY(hipMemcpyAsync(vs->d_stats, vs->h_stats, n_queries * sizeof(value_stats_rec), hipMemcpyHostToDevice, s));
    if (vs->n_edges) HIP_TRY(hipMemcpyAsync(vs->d_edges, vs->edges, size_t(vs->n_edges) * 4, hipMemcpyHostToDevice, s));
    if (n_rows + n_hits) HIP_TRY(hipMemsetAsync(vs->d_rows, 0, (n_rows + n_hits) * 4, s));
    return DINT_OK;
}
// value_stats_kernel over the n_pages pages of qi->cand, in front of ranked_topk; d_page_query[page] + q0: the page's query of
// the call
static int value_stats_launch(const dint_query_index* qi, const value_stats_args* vs, uint64_t n_pages, const uint32_t* d_page_query,
                              uint32_t q0, hipStream_t s) {
    hipLaunchKernelGGL(value_stats_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_pages * kPageSlots, d_page_query, q0,
                       vs->values->view(), vs->d_edges, vs->n_edges, vs->d_stats, vs->d_rows);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// hit_values_kernel behind ranked_topk, over the keys it selected for the n_ids queries from q0 on (qi->topk_out). A call that
// asks for no hit values launches nothing.
static int hit_values_launch(const dint_query_index* qi, const value_stats_args* vs, size_t n_ids, uint32_t q0, hipStream_t s) {
    if (!vs->h_hit_values) return DINT_OK;
    const uint64_t n_out = uint64_t(n_ids) * vs->k;
    hipLaunchKernelGGL(hit_values_kernel, dim3(uint32_t((n_out + 255) / 256)), dim3(256), 0, s, qi->topk_out.p, uint32_t(n_ids), vs->k, q0,
                       vs->values->view(), vs->d_hit_values);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the records', the rows' and the hit values' way back, on the stream, in front of the call's last wait
static int value_stats_back(const value_stats_args* vs, size_t n_queries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(vs->h_stats, vs->d_stats, n_queries * sizeof(value_stats_rec), hipMemcpyDeviceToHost, s));
    if (vs->n_edges) HIP_TRY(hipMemcpyAsync(vs->h_rows, vs->d_rows, vs->row_words(n_queries) * 4, hipMemcpyDeviceToHost, s));
    if (vs->h_hit_values)
        HIP_TRY(hipMemcpyAsync(vs->h_hit_values, vs->d_hit_values, vs->hit_words(n_queries) * 4, hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A group-stats call (hip_api_group_stats.inc): the map and the column, where the call's records go on the host —
// n_queries * n_groups of them, query by query — and where they live on the device: a grow-only workspace of the query index
// of its own, 24 bytes per (query, group). The records go up as the empty record once per call under the lock
// (group_stats_clear), every pass adds, and they come back once. Where a call takes a null one nothing is planned or launched
// differently.
struct group_stats_args {
    const dint_doc_facets* facets = nullptr;
    const dint_doc_values* values = nullptr;
    dint_value_stats* h_recs = nullptr;  // the caller's group_stats
    value_stats_rec* d_recs = nullptr;   // (set by group_stats_clear)
    size_t recs(size_t n_queries) const { return n_queries * size_t(facets->n_groups); }
};
// the call is planned and has refused nothing: every record is empty until a pass says otherwise
static void group_stats_begin(const group_stats_args* gs, size_t n_queries) {
    if (gs) std::fill(gs->h_recs, gs->h_recs + gs->recs(n_queries), dint_value_stats{0, 0, 0xFFFFFFFFu, 0});
}
// under the index's lock, once per call, in front of its first launch: the empty records (the caller's own, as
// group_stats_begin left them) go up
static int group_stats_clear(dint_query_index* qi, group_stats_args* gs, size_t n_queries, hipStream_t s) {
    if (!qi->group_stats_recs.ensure(3 * gs->recs(n_queries))) return DINT_ERR_HIP;
    gs->d_recs = reinterpret_cast<value_stats_rec*>(qi->group_stats_recs.p);
    // (pageable host memory: the copy has left the caller's array when the call returns, and the call waits on the stream
    // before it does)
    HIP_TRY(hipMemcpyAsync(gs->d_recs, gs->h_recs, gs->recs(n_queries) * sizeof(value_stats_rec), hipMemcpyHostToDevice, s));
    return DINT_OK;
}
// group_stats_kernel over the n_pages pages of qi->cand, in front of ranked_topk; d_page_query[page] + q0: the page's query of
// the call
static int group_stats_launch(const dint_query_index* qi, const group_stats_args* gs, uint64_t n_pages, const uint32_t* d_page_query,
                              uint32_t q0, hipStream_t s) {
    hipLaunchKernelGGL(group_stats_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_pages * kPageSlots, d_page_query, q0,
                       gs->facets->view(), gs->values->view(), gs->d_recs);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the records' way back, on the stream, in front of the call's last wait
static int group_stats_back(const group_stats_args* gs, size_t n_queries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(gs->h_recs, gs->d_recs, gs->recs(n_queries) * sizeof(value_stats_rec), hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// A percentile call (hip_api_percentiles.inc): the column and the caller's ranks in parts per million, where the call's
// counts and values go on the host, and where the select lives on the device — two grow-only workspaces of the query index:
// the counter rows, 1 KiB per (query, percentile), and behind one another the copy of per_million, per (query, percentile)
// the state {prefix, rank} and the answer, and per query the valued matches. per_million goes up and the states, the answers
// and the counts are cleared once per call under the lock (percentile_clear); a pass clears its own queries' rows, runs the
// four rounds of its queries to their end (percentile_launch), and everything comes back once. Where a call takes a null one
// nothing is planned or launched differently.
struct percentile_args {
    const dint_doc_values* values = nullptr;
    const uint32_t* per_million = nullptr;  // host, n_p words, each <= 1000000 (checked by the entry)
    uint32_t n_p = 0;
    uint64_t* h_value_counts = nullptr;  // the caller's, n_queries
    uint32_t* h_values = nullptr;        // the caller's percentile_values, n_queries * n_p
    std::vector<uint32_t> h_n;           // out: per query the valued matches, a word each (the entry widens them)
    uint32_t *d_per_million = nullptr, *d_out = nullptr, *d_n = nullptr, *d_rows = nullptr;  // (set by percentile_clear)
    percentile_state* d_state = nullptr;
    size_t recs(size_t n_queries) const { return n_queries * size_t(n_p); }
};
// the call is planned and has refused nothing: no query has a valued match, every percentile is 0 until a pass says otherwise
static void percentile_begin(percentile_args* pa, size_t n_queries) {
    if (!pa) return;
    pa->h_n.assign(n_queries, 0u);
    std::fill(pa->h_value_counts, pa->h_value_counts + n_queries, uint64_t(0));
    std::fill(pa->h_values, pa->h_values + pa->recs(n_queries), 0u);
}
// under the index's lock, once per call, in front of its first launch: per_million goes up, the states, the answers and the
// counts clear
static int percentile_clear(dint_query_index* qi, percentile_args* pa, size_t n_queries, hipStream_t s) {
    const size_t n_recs = pa->recs(n_queries);
    if (!qi->percentile_rows.ensure(n_recs * kPercentileBins) || !qi->percentile_words.ensure(pa->n_p + 3 * n_recs + n_queries))
        return DINT_ERR_HIP;
    pa->d_rows = qi->percentile_rows.p;
    pa->d_per_million = qi->percentile_words.p;
    pa->d_state = reinterpret_cast<percentile_state*>(pa->d_per_million + pa->n_p);
    pa->d_out = pa->d_per_million + pa->n_p + 2 * n_recs;
    pa->d_n = pa->d_out + n_recs;
    // (pageable host memory: the copy has left the caller's array when the call returns, and the call waits on the stream
    // before it does)
    HIP_TRY(hipMemcpyAsync(pa->d_per_million, pa->per_million, size_t(pa->n_p) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(pa->d_state, 0, (3 * n_recs + n_queries) * 4, s));
    return DINT_OK;
}
// The select over the n_pages pages of qi->cand, in front of ranked_topk; d_page_query[page] + q0: the page's query of the
// call, and the pass holds the n_ids whole queries from q0 on. Four rounds of percentile_hist_kernel and
// percentile_resolve_kernel, all on the stream: a round reads the states the round before it left on the device. The rows of
// the pass's queries are cleared in front of round 0 and, since the queries' percentiles share a row there, in front of
// round 1; the resolving waves of rounds 1 and 2 clear the row they alone have read.
static int percentile_launch(const dint_query_index* qi, const percentile_args* pa, uint64_t n_pages, const uint32_t* d_page_query, uint32_t q0,
                             size_t n_ids, hipStream_t s) {
    const size_t n_waves = n_ids * pa->n_p;
    uint32_t* const pass_rows = pa->d_rows + pa->recs(q0) * kPercentileBins;
    for (uint32_t round = 0; round != kPercentileRounds; ++round) {
        if (round < 2) HIP_TRY(hipMemsetAsync(pass_rows, 0, n_waves * kPercentileBins * 4, s));
        hipLaunchKernelGGL(percentile_hist_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_pages * kPageSlots,
                           d_page_query, q0, pa->values->view(), round, pa->n_p, pa->d_state, pa->d_rows);
        hipLaunchKernelGGL(percentile_resolve_kernel, dim3(uint32_t((n_waves + 3) / 4)), dim3(256), 0, s, pa->d_rows, q0, uint32_t(n_ids),
                           pa->n_p, round, pa->d_per_million, pa->d_state, pa->d_n, pa->d_out, round == 1 || round == 2 ? 1u : 0u);
    }
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the counts' and the answers' way back, on the stream, in front of the call's last wait
static int percentile_back(percentile_args* pa, size_t n_queries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(pa->h_n.data(), pa->d_n, n_queries * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(pa->h_values, pa->d_out, pa->recs(n_queries) * 4, hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// The runs and tasks of a selection over the pages of a pass (ranked_topk over the candidate slots, top_values_launch over
// the hash tables): query q's pages are the pages p with page_query[p] == q (consecutive), a page holds page_words keys, and
// the query's keys are cut into runs of R. Pass 0 sorts every run; pass p >= 1 merges run a + 2^(p-1) into run a, a = 0, 2^p,
// 2 * 2^p, ..., until run 0 of every query holds its best R. words(): the tables as the kernels read them (topk_layout).
struct topk_runs {
    std::vector<uint32_t> page_first, pages;
    std::vector<unsigned long long> key_base;
    std::vector<topk_task> tasks;
    std::vector<size_t> pass_first;
    uint64_t n_keys = 0;
    topk_runs(const std::vector<uint32_t>& page_query, size_t n_queries, uint32_t page_words, uint32_t R, bool with_tasks = true)
        : page_first(n_queries, 0), pages(n_queries, 0), key_base(n_queries, 0), pass_first(1, 0) {
        for (size_t p = 0; p != page_query.size(); ++p) {
            const uint32_t q = page_query[p];
            if (pages[q] == 0) page_first[q] = uint32_t(p);
            pages[q] += 1;
        }
        if (!with_tasks) return;
        std::vector<uint32_t> runs(n_queries, 0);
        uint32_t most_runs = 0;
        for (size_t q = 0; q != n_queries; ++q) {
            runs[q] = uint32_t((uint64_t(pages[q]) * page_words + R - 1) / R);
            key_base[q] = n_keys;
            n_keys += uint64_t(runs[q]) * R;
            most_runs = std::max(most_runs, runs[q]);
        }
        for (size_t q = 0; q != n_queries; ++q)
            for (uint32_t a = 0; a != runs[q]; ++a) tasks.push_back({uint32_t(q), a, 0u});
        pass_first.push_back(tasks.size());
        for (uint64_t half = 1; half < most_runs; half <<= 1) {
            for (size_t q = 0; q != n_queries; ++q)
                for (uint64_t a = 0; a + half < runs[q]; a += 2 * half) tasks.push_back({uint32_t(q), uint32_t(a), uint32_t(a + half)});
            pass_first.push_back(tasks.size());
        }
    }
    std::vector<uint32_t> words(const topk_layout& L) const {
        std::vector<uint32_t> h(L.words, 0);
        if (!tasks.empty()) std::memcpy(staged(h.data(), L.tasks), tasks.data(), tasks.size() * sizeof(topk_task));
        if (!pages.empty()) {
            std::memcpy(staged(h.data(), L.page_first), page_first.data(), pages.size() * 4);
            std::memcpy(staged(h.data(), L.pages), pages.data(), pages.size() * 4);
            std::memcpy(staged(h.data(), L.key_base), key_base.data(), pages.size() * 8);
        }
        return h;
    }
};

// A top-values call (hip_api_top_values.inc): the column and how many of its values the caller takes per query, and where the
// call's results live on the device — grow-only workspaces of the query index: per query of the call its valued matches and
// its distinct values, a word each, and the call's overflow word behind them; per (query, i) the selected key; and, per pass,
// the hash tables of the pass's queries (two 64-bit words per slot: a query of P pages owns the 512 P words from word 512 *
// its first page on) and a selection's tasks and keys of their own — ranked_topk runs later on the same stream. The counters,
// the overflow word and the keys are cleared once per call under the lock (top_values_clear); a pass clears its tables,
// counts and selects (top_values_launch), and everything comes back once. Where a call takes a null one nothing is planned or
// launched differently.
struct top_values_args {
    const dint_doc_values* values = nullptr;
    uint32_t n_top = 0;
    std::vector<uint32_t> h_words;            // out: per query the valued matches, per query the distinct values, the overflow word
    std::vector<unsigned long long> h_keys;   // out: n_queries * n_top selected keys, count << 32 | ~value, 0 past a query's last
    std::vector<std::vector<uint32_t>> sent;  // a pass's tables on their way up (pageable: kept until the call's last wait)
    uint32_t *d_n = nullptr, *d_distinct = nullptr, *d_overflow = nullptr;  // (set by top_values_clear)
    unsigned long long* d_out = nullptr;
};
// the call is planned and has refused nothing: no query has a valued match or a value until a pass says otherwise
static void top_values_begin(top_values_args* tv, size_t n_queries) {
    if (!tv) return;
    tv->h_words.assign(2 * n_queries + 1, 0u);
    tv->h_keys.assign(n_queries * tv->n_top, 0ull);
}
// under the index's lock, once per call, in front of its first launch: the counters, the overflow word and the keys clear
static int top_values_clear(dint_query_index* qi, top_values_args* tv, size_t n_queries, hipStream_t s) {
    const size_t n_out = n_queries * tv->n_top;
    if (!qi->top_values_words.ensure(2 * n_queries + 1) || !qi->top_values_out.ensure(std::max<size_t>(1, n_out))) return DINT_ERR_HIP;
    tv->d_n = qi->top_values_words.p;
    tv->d_distinct = tv->d_n + n_queries;
    tv->d_overflow = tv->d_distinct + n_queries;
    tv->d_out = qi->top_values_out.p;
    HIP_TRY(hipMemsetAsync(tv->d_n, 0, (2 * n_queries + 1) * 4, s));
    if (n_out) HIP_TRY(hipMemsetAsync(tv->d_out, 0, n_out * sizeof(unsigned long long), s));
    return DINT_OK;
}
// The count and the selection over the n_pages pages of qi->cand, in front of ranked_topk; page_query[page] (the host's copy
// of d_page_query) + q0: the page's query of the call, and the pass holds the n_ids whole queries from q0 on. On the stream:
// the pass's tables of runs go up, its hash tables clear, top_values_count_kernel fills them, and — n_top != 0 —
// top_values_sort_runs_kernel, the passes of topk_merge_kernel and topk_out_kernel select every query's n_top best words into
// the call's keys at the pass's offset. R = max(256, the power of two >= n_top) divides no table unevenly but for R = 1024 and
// an odd number of pages: the words past the capacity count as empty.
static int top_values_launch(dint_query_index* qi, top_values_args* tv, uint64_t n_pages, const std::vector<uint32_t>& page_query,
                             const uint32_t* d_page_query, uint32_t q0, size_t n_ids, hipStream_t s) {
    uint32_t R = kPageSlots;
    while (R < tv->n_top) R <<= 1;
    const topk_runs runs(page_query, n_ids, kTopValuesPageWords, R, tv->n_top != 0);
    for (uint32_t pages : runs.pages)
        if (uint64_t(pages) * kTopValuesPageWords > 0xFFFFFFFFull) return DINT_ERR_NOMEM;  // (a capacity is a word on the device)
    const topk_layout L(runs.tasks.size(), n_ids);
    const uint64_t n_words = n_pages * kTopValuesPageWords;
    if (!qi->top_values_in.ensure(L.words) || !qi->top_values_table.ensure(n_words) ||
        !qi->top_values_keys.ensure(std::max<uint64_t>(1, runs.n_keys)))
        return DINT_ERR_HIP;
    tv->sent.push_back(runs.words(L));
    HIP_TRY(hipMemcpyAsync(qi->top_values_in.p, tv->sent.back().data(), L.words * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(qi->top_values_table.p, 0, n_words * sizeof(unsigned long long), s));
    const topk_task* const d_tasks = staged<const topk_task>(qi->top_values_in.p, L.tasks);
    const uint32_t* const d_page_first = staged(qi->top_values_in.p, L.page_first);
    const uint32_t* const d_pages = staged(qi->top_values_in.p, L.pages);
    const unsigned long long* const d_base = staged<const unsigned long long>(qi->top_values_in.p, L.key_base);
    hipLaunchKernelGGL(top_values_count_kernel, dim3(uint32_t(n_pages)), dim3(kPageSlots), 0, s, qi->cand.p, n_pages * kPageSlots, d_page_query,
                       q0, tv->values->view(), d_page_first, d_pages, qi->top_values_table.p, tv->d_n, tv->d_distinct, tv->d_overflow);
    if (tv->n_top == 0) return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
    const uint32_t tb = 256;
    for (size_t p = 0; p + 1 < runs.pass_first.size(); ++p) {
        const size_t n_tasks = runs.pass_first[p + 1] - runs.pass_first[p];
        if (n_tasks == 0) continue;
        if (p == 0)
            hipLaunchKernelGGL(top_values_sort_runs_kernel, dim3(uint32_t(n_tasks)), dim3(tb), R * sizeof(unsigned long long), s, d_tasks,
                               d_page_first, d_pages, d_base, qi->top_values_table.p, R, qi->top_values_keys.p);
        else
            hipLaunchKernelGGL(topk_merge_kernel, dim3(uint32_t(n_tasks)), dim3(tb), R * sizeof(unsigned long long), s,
                               d_tasks + runs.pass_first[p], d_base, R, qi->top_values_keys.p);
    }
    const uint64_t n_out = uint64_t(n_ids) * tv->n_top;
    hipLaunchKernelGGL(topk_out_kernel, dim3(uint32_t((n_out + tb - 1) / tb)), dim3(tb), 0, s, d_base, d_pages, qi->top_values_keys.p,
                       uint32_t(n_ids), tv->n_top, tv->d_out + uint64_t(q0) * tv->n_top);
    return hipGetLastError() != hipSuccess ? DINT_ERR_HIP : DINT_OK;
}
// ... and the counters', the overflow word's and the keys' way back, on the stream, in front of the call's last wait
static int top_values_back(top_values_args* tv, size_t n_queries, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(tv->h_words.data(), tv->d_n, (2 * n_queries + 1) * 4, hipMemcpyDeviceToHost, s));
    if (tv->n_top)
        HIP_TRY(hipMemcpyAsync(tv->h_keys.data(), tv->d_out, n_queries * tv->n_top * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    return DINT_OK;
}

// What a ranked call threads through and_queries_impl / or_queries_impl besides its restriction: any of the *_args above, set
// by name, null where the call has none (ca and gl come with fa, and never together). The five steps below are the only place
// that lists them; a call runs them in this order, ranked_topk between the two in the middle. Every step returns the first
// status that is not DINT_OK. AND is one pass over all the call's queries (id0 = 0, n_ids = n_queries); OR runs the two in
// the middle per pass, over the pass's slots in cand and its n_ids whole queries from id0 on.
struct ranked_extras {
    facet_args* fa = nullptr;
    collapse_args* ca = nullptr;
    group_limit_args* gl = nullptr;
    page_args* pg = nullptr;
    sort_args* sv = nullptr;
    value_stats_args* vs = nullptr;
    group_stats_args* gs = nullptr;
    percentile_args* pa = nullptr;
    top_values_args* tv = nullptr;

    // a pass stages its page -> query table for the launches in front of the selection
    bool wants_page_query() const { return fa || pg || sv || vs || gs || pa || tv; }

    // the call is planned and has refused nothing: the host outputs as a call without a match leaves them
    void begin(size_t n_queries) const {
        facet_rows_begin(fa, n_queries);
        collapse_begin(ca, n_queries);
        group_limit_begin(gl, n_queries);
        page_begin(pg, n_queries);
        sort_begin(sv, n_queries);
        value_stats_begin(vs, n_queries);
        group_stats_begin(gs, n_queries);
        percentile_begin(pa, n_queries);
        top_values_begin(tv, n_queries);
    }
    // under the index's lock, once per call, in front of its first launch: the device workspaces sized, sent and cleared
    int clear(dint_query_index* qi, size_t n_queries, hipStream_t s) const {
        int st = DINT_OK;
        if (fa) st = facet_rows_clear(qi, fa, n_queries, s);
        if (ca && st == DINT_OK) st = collapse_clear(qi, ca, fa, n_queries, s);
        if (gl && st == DINT_OK) st = group_limit_clear(qi, gl, fa, n_queries, s);
        if (pg && st == DINT_OK) st = page_begin_device(qi, pg, n_queries, s);
        if (sv && st == DINT_OK) st = sort_begin_device(qi, sv, n_queries, s);
        if (vs && st == DINT_OK) st = value_stats_clear(qi, vs, n_queries, s);
        if (gs && st == DINT_OK) st = group_stats_clear(qi, gs, n_queries, s);
        if (pa && st == DINT_OK) st = percentile_clear(qi, pa, n_queries, s);
        if (tv && st == DINT_OK) st = top_values_clear(qi, tv, n_queries, s);
        return st;
    }
    // The launches in front of ranked_topk, over the n_pages pages of qi->cand; d_page_query[page] + id0: the page's query of
    // the call (page_query: the host's copy, the pass's queries from 0). The one order:
    //  - fa counts every match, so it precedes ca and gl;
    //  - ca and gl precede pg, so the cursor applies to the kept documents;
    //  - the readers (fa, vs, gs, pa, tv) precede those that take slots out of cand (ca, gl, pg, sv), so statistics are over all
    //    matches.
    int before_selection(dint_query_index* qi, uint64_t n_pages, const std::vector<uint32_t>& page_query, const uint32_t* d_page_query,
                         uint32_t id0, size_t n_ids, hipStream_t s) const {
        int st = DINT_OK;
        if (fa) st = facet_count_launch(qi, fa, n_pages, d_page_query, id0, s);
        if (vs && st == DINT_OK) st = value_stats_launch(qi, vs, n_pages, d_page_query, id0, s);
        if (gs && st == DINT_OK) st = group_stats_launch(qi, gs, n_pages, d_page_query, id0, s);
        if (pa && st == DINT_OK) st = percentile_launch(qi, pa, n_pages, d_page_query, id0, n_ids, s);
        if (tv && st == DINT_OK) st = top_values_launch(qi, tv, n_pages, page_query, d_page_query, id0, n_ids, s);
        if (ca && st == DINT_OK) st = collapse_launch(qi, ca, fa, n_pages, d_page_query, id0, s);
        if (gl && st == DINT_OK) st = group_limit_launch(qi, gl, fa, n_pages, d_page_query, id0, s);
        if (pg && st == DINT_OK) st = page_after_launch(qi, pg, n_pages, d_page_query, id0, s);
        if (sv && st == DINT_OK) st = value_after_launch(qi, sv, n_pages, d_page_query, id0, s);
        return st;
    }
    // ... and behind it, over the keys it selected for the n_ids queries (qi->topk_out); no call has two of these
    int after_selection(const dint_query_index* qi, uint64_t n_pages, const uint32_t* d_page_query, uint32_t id0, size_t n_ids,
                        hipStream_t s) const {
        int st = DINT_OK;
        if (ca) st = collapse_hits_launch(qi, ca, fa, n_ids, id0, s);
        if (gl && st == DINT_OK) st = group_limit_hits_launch(qi, gl, fa, n_ids, id0, s);
        if (sv && st == DINT_OK) st = sorted_hits_launch(qi, sv, n_pages, d_page_query, id0, s);
        if (vs && st == DINT_OK) st = hit_values_launch(qi, vs, n_ids, id0, s);
        return st;
    }
    // the way back, on the stream, in front of the call's last wait
    int back(size_t n_queries, hipStream_t s) const {
        int st = DINT_OK;
        if (fa) st = facet_rows_back(fa, n_queries, s);
        if (ca && st == DINT_OK) st = collapse_back(ca, n_queries, s);
        if (gl && st == DINT_OK) st = group_limit_back(gl, n_queries, s);
        if (pg && st == DINT_OK) st = page_back(pg, n_queries, s);
        if (sv && st == DINT_OK) st = sort_back(sv, n_queries, s);
        if (vs && st == DINT_OK) st = value_stats_back(vs, n_queries, s);
        if (gs && st == DINT_OK) st = group_stats_back(gs, n_queries, s);
        if (pa && st == DINT_OK) st = percentile_back(pa, n_queries, s);
        if (tv && st == DINT_OK) st = top_values_back(tv, n_queries, s);
        return st;
    }
};

// the *_queries_freqs entries: a freqs dictionary of the index's device and kind, and somewhere for the sums
static bool freqs_args_ok(const dint_query_index* qi, const dint_dict* freqs_dict, const uint64_t* freq_sums) {
    return freqs_dict && freq_sums && (!qi || (freqs_dict->device == qi->docs->device && freqs_dict->kind == qi->docs->kind));
}

// order[from .. from + n) <- the records from .. from + n - 1 of one query (record from + j: term t[j]) by ascending term
// id: the order its scores are summed in
static void sort_records_by_term(uint32_t* order, uint32_t from, uint32_t n, const uint32_t* t) {
    for (uint32_t j = 0; j != n; ++j) order[from + j] = from + j;
    std::sort(order + from, order + from + n, [&](uint32_t a, uint32_t b) { return t[a - from] < t[b - from]; });
}

// A call cut into passes of whole queries: pass k is the queries [first[k], first[k + 1]). Every size of a pass stays
// within its limit — but a query larger than a limit is a pass alone, sized to it. skip_empty: a query whose sizes are
// all zero never begins a pass.
struct pass_size {
    const uint64_t* of;  // per query
    uint64_t limit;
};
static std::vector<size_t> cut_passes(size_t n_queries, std::initializer_list<pass_size> sizes, bool skip_empty) {
    const pass_size* const sz = sizes.begin();
    const size_t n = sizes.size();
    std::vector<size_t> first(1, 0);
    uint64_t in_pass[4] = {0, 0, 0, 0};  // (per size: at most four)
    for (size_t q = 0; q != n_queries; ++q) {
        bool empty = true, cut = false;
        for (size_t i = 0; i != n; ++i) {
            empty = empty && sz[i].of[q] == 0;
            cut = cut || (in_pass[i] != 0 && in_pass[i] + sz[i].of[q] > sz[i].limit);
        }
        if (skip_empty && empty) continue;
        if (cut) first.push_back(q);
        for (size_t i = 0; i != n; ++i) in_pass[i] = (cut ? 0 : in_pass[i]) + sz[i].of[q];
    }
    first.push_back(n_queries);
    return first;
}
