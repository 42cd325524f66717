// Part of dint_hip.hip (one translation unit; included from there, in order): the handles: a kept bundle schedule (sched_cache), the device dictionary (dint_dict).
// A bundle schedule kept by its owner (a prepared block table: the same units launch after launch) instead of
// being rebuilt, three small kernels, before every launch.
// An in-index schedule may leave a few full blocks to the unit queue (a block that fits no tile: more than 63 lanes of stream —
// 504 bytes of 16-bit slots, 252 of 8-bit ones): up to this many go through a small second launch behind the bundles-only
// kernel; beyond it the general kernel serves the whole table. (A multi-dictionary index of 10^8 postings leaves 8.5 k blocks:
// with the limit at 65536 they took the second launch and the decode was slower, 0.63 against 0.58 ms — profiles/r05_inindex.json.)
constexpr uint32_t kMaxStragglers = DINT_MAX_STRAGGLERS;
#ifndef DINT_INDEX_STRAGGLER_SHARE
#define DINT_INDEX_STRAGGLER_SHARE 32
#endif
constexpr size_t kIndexStragglerShare = DINT_INDEX_STRAGGLER_SHARE;  // in-index tables of kIndexStragglerShareFrom blocks or more: up to 1 / this of the blocks
constexpr size_t kIndexStragglerShareFrom = size_t(1) << 21;
inline size_t index_straggler_limit(size_t n_units) {
    return n_units >= kIndexStragglerShareFrom ? std::max<size_t>(kMaxStragglers, n_units / kIndexStragglerShare) : kMaxStragglers;
}
// ... and a block-granular multi-dictionary unit table (2 * 10^7 units of 256 integers): the few in a thousand that fit no tile
// kept the WHOLE launch on the general kernel (its bundle loop spills; profiles/r05_kernel_stats_multi.csv names it) — up to
// 1/32 of the units follow the bundles-only kernel the same way
inline size_t vroom_straggler_limit(size_t n_units) { return std::max<size_t>(kMaxStragglers, n_units / 32); }
struct sched_cache {
    void* d_mem = nullptr;  // (laid out by sched_layout, hip_stage_layout.inc: the one description, a slot's workspace too)
    size_t mem_bytes = 0;
    bool valid = false;
    // What the schedule was built from. bundle_schedule_kernel bakes this launch's bounds checks (stream bytes, output
    // capacity) and, multi-dictionary streams, the blocks' selector bytes into the unit records: a later launch with
    // another dictionary, stream, unit table, span table or a SMALLER capacity must not reuse them — it rebuilds.
    const void* dict = nullptr;
    const void* d_enc = nullptr;
    const void* d_units = nullptr;
    const void* d_spans = nullptr;
    size_t enc_bytes = 0, n_units = 0, out_capacity = 0;
    uint32_t only_full = 0;
    bool items_known = false;  // n_items has been read back (a prepared unit table does, once)
    uint32_t n_items = 0;      // work items of the unit queue: 0 = every unit is a bundle member
    // round 6 (a prepared multi-dictionary vroom table): the units that fit no tile cut in two records each (split_units_kernel)
    // and scheduled on their own (split_layout, hip_stage_layout.inc) — decoded by a second launch of the bundles kernel;
    // `n_left`: those that could not be cut
    void* d_split = nullptr;
    bool split_ready = false;
    uint32_t n_left = 0;
    bool matches(const void* dd, const void* enc, size_t eb, const void* units, size_t n, const void* spans, size_t cap,
                 uint32_t full) const {
        return valid && dict == dd && d_enc == enc && enc_bytes == eb && d_units == units && n_units == n && d_spans == spans &&
               cap >= out_capacity && only_full == full;
    }
};
// An in-index schedule that has been read back and left at most the stragglers' share to the unit queue: its launches run
// the kernels compiled without the queue (the one-launch decode of a block table asks this of both of its schedules).
inline bool schedule_is_bundles(const sched_cache& c, size_t n_units) {
    return c.valid && c.items_known && c.n_items <= index_straggler_limit(n_units);
}

struct dint_dict {
    int kind = 0;
    int device = 0;
    uint32_t num_dicts = 1;
    uint32_t entries = 0;
    uint32_t compute_units = 0;
    // host copies used by dint_index_stream
    std::vector<uint32_t> h_start;  // per dictionary first meta slot (+ end)
    std::vector<uint32_t> h_size;   // per meta slot
    std::vector<uint32_t> h_hot_k;  // per dictionary: codewords below it have their integers in the LDS image
    std::vector<uint8_t> h_slow;    // per meta slot: a slow entry (not on chip whatever its index)
    uint64_t launches = 0;          // decode launches so far (slot = launch % kQueueSlots)
    // device buffers
    void* d_block = nullptr;  // one allocation: gmeta | rows | gtable | LDS image | descriptors
    uint32_t* d_image = nullptr;
    dint_dev::dict_desc* d_descs = nullptr;
    uint32_t hot_entries = 0;
    uint32_t table_words = 0;
    dint_dev::dict_view view{};
    // timing events of the decode kernel: one pair per queue slot (launches on different streams may
    // interleave); dint_last_kernel_ms reads the pair of the most recent launch
    int last_slot = -1;
    // work-queue counters: one slot per in-flight launch, recycled round-robin
    // behind the event of the launch that used the slot last
    static constexpr uint32_t kQueueSlots = 64;
    uint32_t* d_queues = nullptr;
    // the bundle schedule of a launch (22 bytes per unit): a few workspaces taken in turn — a launch waits (on the host,
    // normally not at all) until the launch that last used its workspace is done. (One per queue slot was 64
    // allocations of half a gigabyte for a block-granular table of 2e7 units.)
    static constexpr uint32_t kSchedSlots = 4;
    uint8_t* d_sched[kSchedSlots] = {};
    size_t sched_cap[kSchedSlots] = {};
    int sched_user[kSchedSlots] = {-1, -1, -1, -1};  // the queue slot of the launch that used it last
    hipEvent_t slot_done[kQueueSlots] = {};
    hipEvent_t slot_start[kQueueSlots] = {}, slot_stop[kQueueSlots] = {};
    bool slot_used[kQueueSlots] = {};
    const uint32_t* slot_clock[kQueueSlots] = {};  // per slot: the clock word of its launch (the slot's own line of d_queues, or the caller's counters)
    std::atomic<uint32_t> next_slot{0};
    std::mutex launch_mutex;
    // The host-pointer calls (dint_decode_list_host, dint_decode_block_host, dint_list_cache_create): a stream of their
    // own, one pinned and one device buffer that only grow — after the first call of a size no allocation, no
    // device-wide synchronisation, one wait for the stream per call. One call at a time per dictionary (host_mutex).
    std::mutex host_mutex;
    hipStream_t host_stream = nullptr;
    uint8_t* h_pin = nullptr;
    uint8_t* d_host = nullptr;
    size_t h_pin_cap = 0, d_host_cap = 0;
    sched_cache host_sched;  // (memory only: the schedule of a host-pointer call is rebuilt every time — other list, same addresses)
};

