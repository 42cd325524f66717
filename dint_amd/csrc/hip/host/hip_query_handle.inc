// Part of dint_hip.hip (one translation unit; included from there, in order): grow-only device workspaces; the query index handle.
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
    std::mutex mutex;

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

