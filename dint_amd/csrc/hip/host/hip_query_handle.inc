// Part of dint_hip.hip (one translation unit; included from there, in order): grow-only device workspaces; the query index handle; the launch of its decode kernels.
namespace {
template <class T>
struct device_buffer {  // grow-only workspace, freed with its owner (on the current device: the owner sets it)
    T* p = nullptr;
    size_t cap = 0;
    device_buffer() = default;
    device_buffer(const device_buffer&) = delete;
    device_buffer& operator=(const device_buffer&) = delete;
    ~device_buffer() {
        if (p) (void)hipFree(p);
    }
    bool ensure(size_t need) {
        if (need <= cap) return true;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = std::max<size_t>(need + need / 2, 1024);
        if (!hip_ok(counted_malloc(&p, want * sizeof(T)), "counted_malloc(workspace)")) return false;
        cap = want;
        return true;
    }
};
}  // namespace

struct dint_query_index {
    const dint_dict* docs = nullptr;
    int device = 0;  // docs->device, kept: the handle may be destroyed after its dictionary
    const uint8_t* d_index = nullptr;
    size_t index_bytes = 0;
    size_t n_blocks = 0;
    std::vector<uint32_t> list_first;  // n_lists + 1
    std::vector<uint32_t> list_len;    // postings per list
    dint_block_ref* d_blocks = nullptr;
    uint32_t* d_block_max = nullptr;
    std::vector<uint32_t> block_max;  // the host's copy of d_block_max: the ranged calls find their blocks in range here
    uint32_t* d_needed = nullptr;   // n_blocks, zero between rounds
    uint32_t* d_rank = nullptr;     // n_blocks
    uint32_t* d_touched = nullptr;  // n_blocks
    bool claims_dirty = false;        // d_needed may hold claim flags of a call that did not run to its end
    // one call = one host-to-device copy (everything the call's kernels read from the host, staged in pinned memory),
    // one clear (every counter the call's launches count in), the launches, one copy back
    void* h_stage = nullptr;
    void* d_stage = nullptr;
    size_t h_stage_cap = 0;
    device_buffer<uint32_t> inputs;
    device_buffer<uint32_t> cand, target, probe, fprobe, tails, spans, bases;
    device_buffer<dint_block_ref> sub;
    device_buffer<dint_unit> units;
    device_buffer<uint64_t> ends;
    device_buffer<uint8_t> gaps_left;
    device_buffer<unsigned long long> freq_sums;
    device_buffer<uint32_t> freq_counts;  // and_query<true>: per term, the blocks its matches fell into
    // the workgroup-per-query batch form (query_batch_body): per workgroup two sets of claim flags / ranks / touched lists
    // (slot_needed is all zero between calls), the queries' control words
    device_buffer<uint32_t> slot_needed, slot_rank, slot_touched, batch_ctrl;
    size_t slot_needed_clean = 0;  // words of slot_needed known to be zero (the buffer grows: a new one is cleared once)
    bool slots_dirty = false;      // a call that did not run to its end may have left claim flags in slot_needed
    // ranked_and (hip_api_ranked_query.inc): the largest docID of the index + 1 (0: no blocks), per candidate slot the
    // score and k1 * ((1 - b) + b * norm_len), per term and query the q_weight, the selection's tasks and keys
    uint64_t doc_bound = 0;
    device_buffer<float> slot_score, slot_kden, qweights;
    device_buffer<uint32_t> topk_in;
    device_buffer<unsigned long long> topk_keys, topk_out;
    // the pruned ranked OR call (hip_api_ranked_or_maxscore.inc): per claim flag of a pass, the flag and its place in the
    // touched list; the touched blocks; {touched count, per query of the pass its claims}
    device_buffer<uint32_t> ms_flag, ms_rank, ms_touched, ms_count;
    // the ranged ranked AND call (hip_api_ranked_range.inc): per query {lo, hi}
    device_buffer<uint32_t> q_ranges;
    // the faceted ranked calls (hip_api_facets.inc): per query of the call a row of n_groups counters
    device_buffer<uint32_t> facet_rows;
    // the collapsed ranked calls (hip_api_collapse.inc): per (query, group) of the call the best key and behind them per
    // query the kept documents; per slot of a pass its group; per (query, i) the hit's group, then its group's matches
    device_buffer<unsigned long long> collapse_best;
    device_buffer<uint32_t> collapse_slot_group, collapse_hits;
    // the group-limited ranked calls (hip_api_group_limit.inc): per (query, place, group) of the call a key and behind them
    // per query the kept documents; per (query, i) the hit's group, then its group's matches, then its place in the group.
    // The slots' groups of a pass go to collapse_slot_group (written and read under the lock within one pass)
    device_buffer<unsigned long long> group_limit_top;
    device_buffer<uint32_t> group_limit_hits;
    // the paged ranked calls (hip_api_paging.inc): per query of the call the cursor's key and behind them per query the
    // matches that are not after it
    device_buffer<unsigned long long> page_keys;
    // the sorted ranked calls (hip_api_doc_values.inc): per query of the call the cursor's key and behind them per query the
    // matches that are not after it; per query whether it has a cursor and behind them per (query, i) the hit's score
    device_buffer<unsigned long long> sort_keys;
    device_buffer<uint32_t> sort_words;
    // the value-stats ranked calls (hip_api_value_stats.inc): per query of the call its record, three 64-bit words; the
    // call's edges and behind them per query a row of n_edges + 1 counters, then per (query, i) the hit's value
    device_buffer<unsigned long long> value_stats_recs;
    device_buffer<uint32_t> value_stats_words;
    // the group-stats ranked calls (hip_api_group_stats.inc): per (query, group) of the call its record, three 64-bit words
    device_buffer<unsigned long long> group_stats_recs;
    // the percentile ranked calls (hip_api_percentiles.inc): per (query, percentile) of the call a row of 256 counters; the
    // call's per_million and behind them per (query, percentile) the select's state and the answer, then per query its count
    device_buffer<uint32_t> percentile_rows, percentile_words;
    // the top-values ranked calls (hip_api_top_values.inc): per slot of a pass two words of its query's hash table; per query
    // of the call its valued matches, then its distinct values, then the call's overflow word; a selection of their own over
    // the tables — the tasks, the runs' keys and per (query, i) of the call the selected key (the ranked selection runs later
    // on the same stream, in topk_in / topk_keys / topk_out)
    device_buffer<unsigned long long> top_values_table, top_values_keys, top_values_out;
    device_buffer<uint32_t> top_values_words, top_values_in;
    // dint_check_index (hip_api_check.inc): every block of a list but its last holds 256 postings (the in-index layout:
    // block j of a list is its positions [256 j, 256 j + n)); two pinned staging buffers of a pass's expected postings
    // and their device copies, alternating
    bool whole_blocks = true;
    void* h_expect[2] = {nullptr, nullptr};
    size_t h_expect_cap = 0;  // bytes, of each
    device_buffer<uint32_t> expect[2];
    std::mutex mutex;

    uint32_t blocks_of(uint32_t l) const { return list_first[l + 1] - list_first[l]; }
    // a staged field (hip_stage_layout.inc) as the host fills it and as the kernels read it, from its one offset
    template <class T = uint32_t>
    T* h(size_t at) const { return staged<T>(h_stage, at); }
    template <class T = uint32_t>
    T* d(size_t at) const { return staged<T>(inputs.p, at); }
    // h_stage of at least `bytes` (grown by half again), d_stage the same memory as the kernels see it (null where it
    // cannot be mapped)
    hipError_t stage(size_t bytes) {
        if (h_stage_cap >= bytes) return hipSuccess;
        if (h_stage) (void)hipHostFree(h_stage);
        h_stage = nullptr;
        h_stage_cap = 0;
        const size_t want = bytes + bytes / 2 + 4096;
        const hipError_t e = counted_host_malloc(&h_stage, want);
        if (e != hipSuccess) return e;
        h_stage_cap = want;
        d_stage = nullptr;
        if (hipHostGetDevicePointer(&d_stage, h_stage, 0) != hipSuccess) d_stage = nullptr;
        return hipSuccess;
    }
};

namespace {
// What every decode_*_query*_kernel launch starts from: the docs dictionary over the index. with_image false — lists of
// fewer than 256 postings are one interpolative block each and need no dictionary: a query of such lists only (most of
// a query log's) runs without the 88 KB LDS image — nothing reads it.
decode_args query_decode_args(const dint_query_index* qi, bool with_image = true) {
    decode_args a{};
    a.dict = qi->docs->view;
    a.enc = qi->d_index;
    a.enc_bytes = qi->index_bytes;
    if (!with_image) a.dict.hot_words = 0;
    return a;
}
// ... and the launch: the LDS bytes of a's image, the single- or the multi-dictionary kernel
template <class K, class... A>
int query_decode_launch(const dint_query_index* qi, const decode_args& a, uint32_t grid, hipStream_t s, K single, K multi,
                               const A&... args) {
    const size_t lds_bytes = (size_t(a.dict.hot_words) + kClassTableWords + kWavesPerBlock * kScratchWords) * 4;
    hipLaunchKernelGGL(qi->docs->kind == DINT_DICT_MULTI_PACKED ? multi : single, dim3(grid), dim3(kBlockThreads), lds_bytes, s, a, args...);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}
}  // namespace

