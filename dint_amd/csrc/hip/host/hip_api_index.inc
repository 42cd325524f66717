// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the in-index path — dint_index_posting_lists, block tables, dint_decode_block_table / dint_decode_posting_blocks (dict_posting_list.hpp:10-56, 284-318).
int dint_index_posting_lists(const uint8_t* index, size_t index_bytes, const uint64_t* list_offsets,
                             size_t n_lists, dint_block_ref** blocks_out, size_t* n_blocks,
                             uint64_t* total_postings) {
    if ((!index && index_bytes) || (!list_offsets && n_lists) || !blocks_out || !n_blocks) return DINT_ERR_ARG;
    std::vector<dint_block_ref> blocks;
    uint64_t out_pos = 0;
    for (size_t i = 0; i != n_lists; ++i) {
        if (list_offsets[i] >= index_bytes) return DINT_ERR_FORMAT;
        const uint8_t* p = index + list_offsets[i];
        const uint8_t* end = index + index_bytes;
        uint32_t n;
        const uint8_t* base = read_vbyte(p, end, &n);  // document_enumerator ctor, dict_posting_list.hpp:90-107
        if (!base || n == 0) return DINT_ERR_FORMAT;
        const uint64_t nb = (uint64_t(n) + kBlock - 1) / kBlock;
        const uint8_t* maxs = base;
        const uint8_t* endpoints = maxs + 4 * nb;
        const uint8_t* data = endpoints + 4 * (nb - 1);
        if (data > end) return DINT_ERR_FORMAT;
        uint32_t prev_max = uint32_t(-1);
        for (uint64_t b = 0; b != nb; ++b) {
            uint32_t endpoint = 0, mx;
            if (b) std::memcpy(&endpoint, endpoints + 4 * (b - 1), 4);
            std::memcpy(&mx, maxs + 4 * b, 4);
            dint_block_ref r;
            r.in_off = uint64_t(data - index) + endpoint;
            r.out_off = out_pos;
            r.n = (b + 1) * kBlock <= n ? kBlock : n % kBlock;
            r.base = prev_max + 1;
            r.max = mx;
            r.list = uint32_t(i);
            if (r.in_off > index_bytes) return DINT_ERR_FORMAT;
            blocks.push_back(r);
            out_pos += r.n;
            prev_max = mx;
        }
    }
    auto mem = static_cast<dint_block_ref*>(std::malloc(std::max<size_t>(1, blocks.size()) * sizeof(dint_block_ref)));
    if (!mem) return DINT_ERR_NOMEM;
    if (!blocks.empty()) std::memcpy(mem, blocks.data(), blocks.size() * sizeof(dint_block_ref));
    *blocks_out = mem;
    *n_blocks = blocks.size();
    if (total_postings) *total_postings = out_pos;
    return DINT_OK;
}

// A block table prepared for decoding: what depends on the table alone is computed once — the docs parts' unit
// table, byte spans and docID bases, the list of short (interpolative) blocks — and the per-call workspace (where
// the docs parts end, the freqs parts' units) lives here too, so that a decode is a sequence of launches and
// nothing else.
struct dint_block_table {
    int device = 0;
    size_t n_blocks = 0, n_tails = 0;
    bool owns_blocks = false;
    const dint_block_ref* d_blocks = nullptr;
    void* d_ws = nullptr;  // one allocation: everything below
    dint_unit* d_units = nullptr;       // docs parts
    uint32_t* d_spans = nullptr;
    uint32_t* d_bases = nullptr;
    uint32_t* d_tails = nullptr;        // indices of the short blocks, then their number
    uint64_t* d_ends = nullptr;         // per call: where each docs part ended = where the freqs part begins
    dint_unit* d_funits = nullptr;      // per call: freqs parts
    uint32_t* d_fspans = nullptr;
    uint8_t* d_gaps_left = nullptr;     // per call: blocks the decode kernels left as gaps
    // per call: the docs and the freqs launch's counters. Two sets, taken in turn: the one-launch decode clears the other
    // set for the decode after it (tails_args::zero_next); a set not known to be clean is filled on the stream first
    uint32_t* d_counter_sets[2] = {nullptr, nullptr};
    int cur_set = 0;
    bool set_clean[2] = {false, false};
    size_t zero_bytes = 0;              // a set
    bool spans_exact = false;           // the docs parts' byte spans have been cut down to their ends (after the first decode)
    // From the third decode on nothing but the decode kernels, the interpolative decoder and the clean-up run:
    // the first decode learns where the docs parts end (exact spans, the freqs parts' units), the second builds
    // the two bundle schedules from them, and both are a property of the index, not of the call.
    uint32_t decodes = 0;
    sched_cache docs_sched, freqs_sched;
    bool freqs_units_ready = false;
    uint64_t max_out_end = 0;           // max over the blocks of out_off + n: a decode whose out_capacity is below it skips blocks
    // Once the freqs parts' units are known (second decode on), their launch depends on nothing the docs launch produces:
    // it runs on a stream of the table's own, beside the docs launch and the short blocks' decoder, between two events
    // on the caller's stream (each launch is a quarter of a millisecond of persistent workgroups: one's ramp and tail
    // under the other's body).
    hipStream_t side = nullptr, side2 = nullptr;  // (side2: the short blocks' decoder)
    hipEvent_t fork = nullptr, join = nullptr, join2 = nullptr;
    // A table created from blocks the host has seen: its short blocks sorted by length, longest first, and cut into tickets
    // for the docs launch's waves (tails_phase, kernels/index.inc) — no launch of their own then.
    void* d_tail_sched = nullptr;
    uint32_t* d_tail_ids = nullptr;
    u32x2* d_tail_tickets = nullptr;
    uint32_t n_tail_tickets = 0;
};

namespace {
int block_table_prepare(dint_block_table& t, const dint_block_ref* d_blocks, size_t n_blocks, size_t index_bytes, hipStream_t s) {
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_units = up(n_blocks * sizeof(dint_unit)), b_u32 = up((n_blocks + 1) * 4), b_u64 = up(n_blocks * 8),
                 b_u8 = up(n_blocks);
    const size_t b_counters = 2 * size_t(kQueueLines) * kQueueStride * 4;
    HIP_TRY(counted_malloc(&t.d_ws, 2 * b_units + 4 * b_u32 + b_u64 + b_u8 + 2 * b_counters));
    uint8_t* p = static_cast<uint8_t*>(t.d_ws);
    t.d_units = reinterpret_cast<dint_unit*>(p), p += b_units;
    t.d_funits = reinterpret_cast<dint_unit*>(p), p += b_units;
    t.d_ends = reinterpret_cast<uint64_t*>(p), p += b_u64;
    t.d_spans = reinterpret_cast<uint32_t*>(p), p += b_u32;
    t.d_fspans = reinterpret_cast<uint32_t*>(p), p += b_u32;
    t.d_bases = reinterpret_cast<uint32_t*>(p), p += b_u32;
    t.d_tails = reinterpret_cast<uint32_t*>(p), p += b_u32;
    t.d_gaps_left = p;
    t.d_counter_sets[0] = reinterpret_cast<uint32_t*>(p + b_u8);
    t.d_counter_sets[1] = reinterpret_cast<uint32_t*>(p + b_u8 + b_counters);
    t.zero_bytes = b_counters;
    t.d_blocks = d_blocks;
    t.n_blocks = n_blocks;
    const uint32_t tb = 256, grid = uint32_t((n_blocks + tb - 1) / tb);
    HIP_TRY(hipMemsetAsync(t.d_tails + n_blocks, 0, 4, s));
    HIP_TRY(hipMemsetAsync(t.d_ends, 0, n_blocks * 8, s));  // (a block a decode skips leaves its end offset untouched)
    hipLaunchKernelGGL(collect_tails_kernel, dim3(grid), dim3(tb), 0, s, d_blocks, uint64_t(n_blocks), t.d_tails, t.d_tails + n_blocks);
    hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, d_blocks, static_cast<const uint64_t*>(nullptr),
                       uint64_t(n_blocks), uint64_t(index_bytes), t.d_units, t.d_spans, t.d_bases);
    HIP_TRY(hipGetLastError());
    uint32_t n_tails = 0;
    HIP_TRY(hipMemcpyAsync(&n_tails, t.d_tails + n_blocks, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    t.n_tails = n_tails;
    return DINT_OK;
}

// One decode call of a block table, as its two forms see it: the docs and the freqs launch (the same request over the
// blocks, each with its own units, spans, output, schedule and half of the call's counters) and what the call decided.
struct block_decode {
    dint_block_table& t;
    decode_request docs, freqs;  // (freqs.out null: docs only)
    tails_args sb{};             // the short blocks' tickets where the docs launch brings them along (tails_phase), else empty
    bool inline_tails = false;
    bool covers = false;         // this call decodes EVERY block
    bool keep = false;           // what the call learns is kept for the next ones
    bool concurrent = false;     // ... and the table's side streams may be used
    explicit block_decode(dint_block_table& table) : t(table) {}
};

// The table's two side streams and three events: all five or none (a table with half of them would trip over the missing
// ones on its next decode).
int ensure_side_streams(dint_block_table& t) {
    if (t.side) return DINT_OK;
    hipStream_t s1 = nullptr, s2 = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    int prio_low = 0, prio_high = 0;  // (the short blocks' few, long-lived waves first: the DINT launches fill in around them)
    const bool ok = hip_ok(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking), "hipStreamCreateWithFlags") &&
                    hip_ok(hipDeviceGetStreamPriorityRange(&prio_low, &prio_high), "hipDeviceGetStreamPriorityRange") &&
                    hip_ok(hipStreamCreateWithPriority(&s2, hipStreamNonBlocking, prio_high), "hipStreamCreateWithPriority") &&
                    hip_ok(hipEventCreateWithFlags(&e0, hipEventDisableTiming), "hipEventCreateWithFlags") &&
                    hip_ok(hipEventCreateWithFlags(&e1, hipEventDisableTiming), "hipEventCreateWithFlags") &&
                    hip_ok(hipEventCreateWithFlags(&e2, hipEventDisableTiming), "hipEventCreateWithFlags");
    if (!ok) {
        if (s1) (void)hipStreamDestroy(s1);
        if (s2) (void)hipStreamDestroy(s2);
        for (hipEvent_t e : {e0, e1, e2})
            if (e) (void)hipEventDestroy(e);
        return DINT_ERR_HIP;
    }
    t.side = s1, t.side2 = s2, t.fork = e0, t.join = e1, t.join2 = e2;
    return DINT_OK;
}

// The short blocks — both parts of a block in one lane — through the interpolative decoder, a launch of their own
// (one wave per kTailLanes short blocks; their outputs are their own)
void launch_short_blocks(const dint_block_table& t, hipStream_t s, const block_decode& c) {
    const uint32_t tgrid = uint32_t((t.n_tails + kTailLanes - 1) / kTailLanes);
    hipLaunchKernelGGL(interpolative_tails_kernel, dim3(tgrid), dim3(64), kTailLdsBytes, s, c.docs.enc, uint64_t(c.docs.enc_bytes), t.d_blocks,
                       static_cast<const uint64_t*>(nullptr), t.d_tails, t.d_tails + t.n_blocks, c.docs.out, uint64_t(c.docs.out_capacity),
                       static_cast<uint64_t*>(nullptr), 0u, 1u, c.freqs.out, static_cast<uint8_t*>(nullptr), uint64_t(0));
}

// ONE launch for the docs parts, the short blocks and the freqs parts (decode_*_index_pair_kernel): both kept schedules
// are known to be bundles and nothing else (or nearly: the stragglers' small launches follow).
int block_table_decode_pair(block_decode& c) {
    dint_block_table& t = c.t;
    hipStream_t s = c.docs.stream;
    deferred_launch pd, pf;
    c.docs.defer = &pd;
    c.freqs.defer = &pf;
    int st = launch_decode(c.docs);
    if (st != DINT_OK) return st;
    st = launch_decode(c.freqs);
    if (st != DINT_OK) {
        if (pd.prepared) (void)finish_deferred(pd);
        return st;
    }
    tails_args sb = c.sb;
    if (pd.prepared && pf.prepared && pd.bundles_only && pf.bundles_only && pd.grid == pf.grid) {
        const size_t lds = std::max(pd.lds_bytes, pf.lds_bytes);
        sb.zero_next = t.d_counter_sets[t.cur_set ^ 1];  // (the next decode's counters: see tails_args)
        sb.zero_words = uint32_t(t.zero_bytes / 4);
        hipLaunchKernelGGL(pd.dict->kind == DINT_DICT_MULTI_PACKED ? decode_multi_index_pair_kernel : decode_single_index_pair_kernel,
                           dim3(pd.grid), dim3(kBlockThreads), lds, s, pd.a, pf.a, sb);
    } else {  // (a schedule was rebuilt under this call: a launch each)
        if (pd.prepared) launch_prepared(pd);
        if (pf.prepared) launch_prepared(pf);
    }
    if (pd.prepared) launch_stragglers(pd);
    if (pf.prepared) launch_stragglers(pf);
    if (pd.prepared) st = finish_deferred(pd);
    if (st == DINT_OK && pf.prepared) st = finish_deferred(pf);
    if (st != DINT_OK) return st;
    HIP_TRY(hipGetLastError());
    if (sb.zero_next != nullptr) {  // (the launch that clears the other set is on the stream)
        t.set_clean[t.cur_set ^ 1] = true;
        t.cur_set ^= 1;
    }
    if (c.covers) t.decodes += 1;
    return DINT_OK;
}

// A launch each: docs parts of the full blocks through the DINT kernel (docIDs formed in the expansion); then, where they
// end, their freqs parts; the short blocks inside the docs launch or through a launch of their own. From the second decode
// of a table on (the side streams are the table's) the freqs launch runs beside the docs launch once its units are known,
// and the short blocks' decoder beside both.
int block_table_decode_each(block_decode& c) {
    dint_block_table& t = c.t;
    hipStream_t s = c.docs.stream;
    const size_t n_blocks = t.n_blocks;
    const uint32_t tb = 256, grid = uint32_t((n_blocks + tb - 1) / tb);
    const bool with_freqs = c.freqs.out != nullptr;
    const bool tails_apart = t.n_tails != 0 && !c.inline_tails;
    const bool side_freqs = with_freqs && t.freqs_units_ready && c.concurrent;
    const bool side_tails = tails_apart && c.concurrent;
    if (side_freqs || side_tails) {
        const int st = ensure_side_streams(t);
        if (st != DINT_OK) return st;
        HIP_TRY(hipEventRecord(t.fork, s));  // (what the caller put on its stream before this call — the index — is there)
    }
    if (side_freqs) {
        c.freqs.stream = t.side;  // (its counters were cleared on the caller's stream, before the fork)
        HIP_TRY(hipStreamWaitEvent(t.side, t.fork, 0));
    }
    hipStream_t fs = c.freqs.stream;
    if (side_tails) {
        HIP_TRY(hipStreamWaitEvent(t.side2, t.fork, 0));
        launch_short_blocks(t, t.side2, c);
        HIP_TRY(hipEventRecord(t.join2, t.side2));
    }
    auto fail = [&](int code) {  // (nothing of this call may still be running on the table's streams when the caller hears of it)
        if (side_freqs) (void)hipStreamSynchronize(t.side);
        if (side_tails) (void)hipStreamSynchronize(t.side2);
        return code;
    };
    int st = launch_decode(c.docs);
    if (st != DINT_OK) return fail(st);
    if (!t.spans_exact && c.covers) {  // (stream-ordered: the next decode on this table finds the exact spans)
        hipLaunchKernelGGL(exact_spans_kernel, dim3(grid), dim3(tb), 0, s, t.d_units, t.d_ends, uint64_t(n_blocks), t.d_spans);
        t.spans_exact = true;
    }
    if (with_freqs) {
        if (!t.freqs_units_ready) {
            // (a skipped block's end offset is zero: its freqs unit then starts at the buffer's first byte and is
            // skipped in turn — same out_off, same capacity)
            hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, t.d_blocks, t.d_ends, uint64_t(n_blocks),
                               uint64_t(c.docs.enc_bytes), t.d_funits, t.d_fspans, static_cast<uint32_t*>(nullptr));
            t.freqs_units_ready = t.owns_blocks && c.covers;
        }
        st = launch_decode(c.freqs);
        if (st != DINT_OK) return fail(st);
        if (fs != s) HIP_TRY(hipEventRecord(t.join, fs));
    }
    if (side_tails) {
        HIP_TRY(hipStreamWaitEvent(s, t.join2, 0));
    } else if (tails_apart)
        launch_short_blocks(t, s, c);
    HIP_TRY(hipGetLastError());
    if (fs != s) HIP_TRY(hipStreamWaitEvent(s, t.join, 0));  // (everything behind this call on the caller's stream sees the freqs)
    // Once per kept schedule (the decode that built it): how many work items its unit queue got.
    if (c.keep) {
        st = read_queue_items(t.docs_sched, n_blocks, s);
        if (st == DINT_OK && with_freqs) st = read_queue_items(t.freqs_sched, n_blocks, fs);
        if (st != DINT_OK) return fail(st);
    }
    if (c.covers) t.decodes += 1;
    return DINT_OK;
}

// docs parts -> docIDs, freqs parts -> freqs: launches only, nothing waited for
int block_table_decode(const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index, size_t index_bytes,
                       dint_block_table& t, uint32_t* d_docids, uint32_t* d_freqs, size_t out_capacity, hipStream_t s) {
    // ONE fill: the two launches' counters. (The "left as gaps" flags need none: a flag is the decoding wave's own — cleared,
    // perhaps set, looked at and cleared again by the wave that decodes the block, which turns the rare block it had to
    // leave as gaps into docIDs on the spot: gaps_to_docids_here. Until round 4 the flags were cleared per call and a
    // fix-up launch went through them behind the decode: two fills and a launch of 9 us behind a 20 us gap.)
    uint32_t* const d_counters = t.d_counter_sets[t.cur_set];
    if (!t.set_clean[t.cur_set]) HIP_TRY(hipMemsetAsync(d_counters, 0, t.zero_bytes, s));
    t.set_clean[t.cur_set] = false;  // (in use from here on)
    block_decode c(t);
    // What a decode learns for the next ones (exact spans, the freqs parts' units, the schedules) is kept only when
    // this call decodes EVERY block: with an out_capacity below some block's end the kernels skip that block and leave
    // its end offset unwritten — nothing may be derived from it.
    c.covers = out_capacity >= t.max_out_end;
    c.keep = t.owns_blocks && c.covers && t.decodes >= 1;  // (a one-shot table never reaches its second decode)
    const bool concurrent_ok = opt(DINT_OPT_INDEX_CONCURRENT) != 0;
    c.concurrent = c.keep && concurrent_ok;
    c.inline_tails = t.n_tail_tickets != 0 && opt(DINT_OPT_INDEX_INLINE_TAILS) != 0;
    if (c.inline_tails) {
        c.sb.blocks = t.d_blocks, c.sb.ids = t.d_tail_ids, c.sb.tickets = t.d_tail_tickets, c.sb.n_tickets = t.n_tail_tickets;
        c.sb.docids = d_docids, c.sb.freqs = d_freqs, c.sb.out_capacity = out_capacity;
    }
    decode_request blocks;  // what the two launches share
    blocks.enc = d_index, blocks.enc_bytes = index_bytes, blocks.n_units = t.n_blocks, blocks.out_capacity = out_capacity;
    blocks.stream = s, blocks.only_full = 1;
    c.docs = c.freqs = blocks;
    c.docs.dict = docs_dict, c.docs.units = t.d_units, c.docs.spans = t.d_spans, c.docs.out = d_docids;
    c.docs.cache = c.keep ? &t.docs_sched : nullptr, c.docs.own_counters = d_counters;
    c.docs.end_off = t.d_ends, c.docs.unit_base = t.d_bases, c.docs.gaps_left = t.d_gaps_left;
    c.docs.short_blocks = c.inline_tails ? &c.sb : nullptr;
    c.freqs.dict = freqs_dict, c.freqs.units = t.d_funits, c.freqs.spans = t.d_fspans, c.freqs.out = d_freqs;
    c.freqs.cache = c.keep ? &t.freqs_sched : nullptr, c.freqs.own_counters = d_counters + size_t(kQueueLines) * kQueueStride;
    c.freqs.plus_one = 1;  // (freq = decoded value + 1, dict_posting_list.hpp:164-169: added where the values are stored)
    const bool pair = d_freqs && c.concurrent && t.freqs_units_ready && t.spans_exact && (t.n_tails == 0 || c.inline_tails) &&
                      opt(DINT_OPT_INDEX_PAIR) != 0 && schedule_is_bundles(t.docs_sched, t.n_blocks) &&
                      schedule_is_bundles(t.freqs_sched, t.n_blocks) && docs_dict->kind == freqs_dict->kind;
    return pair ? block_table_decode_pair(c) : block_table_decode_each(c);
}
}  // namespace

int dint_block_table_create(const dint_dict* docs_dict, const dint_block_ref* blocks, size_t n_blocks, size_t index_bytes,
                            dint_block_table** out) {
    if (!docs_dict || !out || (!blocks && n_blocks)) return DINT_ERR_ARG;
    *out = nullptr;
    if (n_blocks >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    uint64_t max_out_end = 0;
    for (size_t b = 0; b != n_blocks; ++b) {
        if (blocks[b].n == 0 || blocks[b].n > kBlock || blocks[b].in_off > index_bytes) return DINT_ERR_FORMAT;
        if (blocks[b].out_off + blocks[b].n >= blocks[b].out_off) max_out_end = std::max<uint64_t>(max_out_end, blocks[b].out_off + blocks[b].n);
        else max_out_end = ~uint64_t(0);  // (wraps: no capacity covers it)
    }
    auto* t = new (std::nothrow) dint_block_table();
    if (!t) return DINT_ERR_NOMEM;
    t->device = docs_dict->device;
    t->max_out_end = max_out_end;
    if (n_blocks == 0) {
        *out = t;
        return DINT_OK;
    }
    dint_block_ref* d_blocks = nullptr;
    int st = DINT_ERR_HIP;
    if (hip_ok(hipSetDevice(t->device), "hipSetDevice") && hip_ok(counted_malloc(&d_blocks, n_blocks * sizeof(dint_block_ref)), "counted_malloc(blocks)") &&
        hip_ok(hipMemcpy(d_blocks, blocks, n_blocks * sizeof(dint_block_ref), hipMemcpyHostToDevice), "hipMemcpy(blocks)")) {
        t->owns_blocks = true;
        st = block_table_prepare(*t, d_blocks, n_blocks, index_bytes, nullptr);
        if (st == DINT_OK) {  // the short blocks' tickets (tails_phase): longest first, one lane each, as many as fit a wave's scratch
            std::vector<uint32_t> ids;
            for (size_t b = 0; b != n_blocks; ++b)
                if (blocks[b].n < kBlock) ids.push_back(uint32_t(b));
            std::stable_sort(ids.begin(), ids.end(), [&](uint32_t x, uint32_t y) { return blocks[x].n > blocks[y].n; });
            std::vector<u32x2> tickets;
            for (size_t i = 0; i < ids.size();) {
                uint32_t row = blocks[ids[i]].n + 1 + kTicketStack;
                row |= 1u;  // (odd: the lanes' rows fall into different LDS banks)
                const size_t cnt = std::min<size_t>(std::min<size_t>(kWave, kTicketWords / row), ids.size() - i);
                u32x2 tk;
                tk.x = uint32_t(i);
                tk.y = uint32_t(cnt) | (row << 8);
                tickets.push_back(tk);
                i += cnt;
            }
            if (!tickets.empty()) {
                const size_t b_ids = (ids.size() * 4 + 255) / 256 * 256;
                st = DINT_ERR_HIP;
                if (hip_ok(counted_malloc(&t->d_tail_sched, b_ids + tickets.size() * sizeof(u32x2)), "counted_malloc(short blocks)")) {
                    t->d_tail_ids = static_cast<uint32_t*>(t->d_tail_sched);
                    t->d_tail_tickets = reinterpret_cast<u32x2*>(static_cast<uint8_t*>(t->d_tail_sched) + b_ids);
                    if (hip_ok(hipMemcpy(t->d_tail_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(short blocks)") &&
                        hip_ok(hipMemcpy(t->d_tail_tickets, tickets.data(), tickets.size() * sizeof(u32x2), hipMemcpyHostToDevice), "hipMemcpy(tickets)")) {
                        t->n_tail_tickets = uint32_t(tickets.size());
                        st = DINT_OK;
                    }
                }
            }
        }
    }
    if (st != DINT_OK) {
        if (d_blocks && !t->d_blocks) (void)hipFree(d_blocks);
        dint_block_table_destroy(t);
        return st;
    }
    *out = t;
    return DINT_OK;
}

void dint_block_table_destroy(dint_block_table* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->d_ws) (void)hipFree(t->d_ws);
    if (t->d_tail_sched) (void)hipFree(t->d_tail_sched);
    if (t->side) {
        (void)hipStreamSynchronize(t->side);
        (void)hipStreamDestroy(t->side);
        (void)hipEventDestroy(t->fork);
        (void)hipEventDestroy(t->join);
        (void)hipStreamSynchronize(t->side2);
        (void)hipStreamDestroy(t->side2);
        (void)hipEventDestroy(t->join2);
    }
    if (t->docs_sched.d_mem) (void)hipFree(t->docs_sched.d_mem);
    if (t->freqs_sched.d_mem) (void)hipFree(t->freqs_sched.d_mem);
    if (t->owns_blocks && t->d_blocks) (void)hipFree(const_cast<dint_block_ref*>(t->d_blocks));
    delete t;
}

int dint_decode_block_table(const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index, size_t index_bytes,
                            dint_block_table* table, uint32_t* d_docids, uint32_t* d_freqs, size_t out_capacity, void* stream) {
    if (!docs_dict || !table || (d_freqs && !freqs_dict)) return DINT_ERR_ARG;
    if (table->n_blocks == 0) return DINT_OK;
    if (!d_index || !d_docids || index_bytes < 8 || table->device != docs_dict->device) return DINT_ERR_ARG;
    if (freqs_dict && (freqs_dict->device != docs_dict->device || freqs_dict->kind != docs_dict->kind)) return DINT_ERR_ARG;
    HIP_TRY(hipSetDevice(docs_dict->device));
    return block_table_decode(docs_dict, freqs_dict, d_index, index_bytes, *table, d_docids, d_freqs, out_capacity,
                              static_cast<hipStream_t>(stream));
}

int dint_block_table_learn(dint_block_table* table, const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index,
                           size_t index_bytes, void* stream) {
    if (!table || !docs_dict) return DINT_ERR_ARG;
    if (table->n_blocks == 0) return DINT_OK;
    if (!table->owns_blocks || !d_index || index_bytes < 8 || table->device != docs_dict->device || table->max_out_end == ~uint64_t(0))
        return DINT_ERR_ARG;
    if (freqs_dict && (freqs_dict->device != docs_dict->device || freqs_dict->kind != docs_dict->kind)) return DINT_ERR_ARG;
    HIP_TRY(hipSetDevice(docs_dict->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cap = size_t(table->max_out_end);
    uint32_t* d_scratch = nullptr;
    HIP_TRY(counted_malloc(&d_scratch, std::max<size_t>(1, cap) * 4 * (freqs_dict ? 2 : 1)));
    // decode 1 learns the spans and the freqs parts' units, decode 2 builds and keeps both schedules (and reads how many
    // work items they left to the unit queue): what the caller's first two decodes used to do, into a scratch output
    int st = DINT_OK;
    for (int pass = 0; pass != 2 && st == DINT_OK; ++pass)
        st = block_table_decode(docs_dict, freqs_dict, d_index, index_bytes, *table, d_scratch, freqs_dict ? d_scratch + cap : nullptr, cap, s);
    const hipError_t e = hipStreamSynchronize(s);
    (void)hipFree(d_scratch);
    if (st != DINT_OK) return st;
    HIP_TRY(e);
    return DINT_OK;
}

int dint_block_table_ready(const dint_block_table* t, int with_freqs) {
    if (!t) return 0;
    if (t->n_blocks == 0) return 1;
    if (!t->owns_blocks || t->decodes < 1 || !t->spans_exact || !schedule_is_bundles(t->docs_sched, t->n_blocks)) return 0;
    return !with_freqs || (t->freqs_units_ready && schedule_is_bundles(t->freqs_sched, t->n_blocks)) ? 1 : 0;
}

int dint_block_table_info_get(const dint_block_table* t, dint_block_table_info* info) {
    if (!t || !info) return DINT_ERR_ARG;
    info->n_blocks = t->n_blocks;
    info->n_short_blocks = t->n_tails;
    info->complete_decodes = t->decodes;
    info->spans_exact = t->spans_exact ? 1u : 0u;
    info->freqs_units_ready = t->freqs_units_ready ? 1u : 0u;
    info->docs_schedule = t->docs_sched.valid && t->docs_sched.items_known ? 1u : 0u;
    info->freqs_schedule = t->freqs_sched.valid && t->freqs_sched.items_known ? 1u : 0u;
    info->docs_queue_items = t->docs_sched.n_items;
    info->freqs_queue_items = t->freqs_sched.n_items;
    info->short_block_tickets = t->n_tail_tickets;
    return DINT_OK;
}

int dint_decode_posting_blocks(const dint_dict* docs_dict, const dint_dict* freqs_dict, const uint8_t* d_index,
                               size_t index_bytes, const dint_block_ref* d_blocks, size_t n_blocks,
                               uint32_t* d_docids, uint32_t* d_freqs, size_t out_capacity, void* stream) {
    if (!docs_dict || (d_freqs && !freqs_dict)) return DINT_ERR_ARG;
    if (n_blocks == 0) return DINT_OK;
    if (!d_index || !d_blocks || !d_docids || index_bytes < 8 || n_blocks >= 0xFFFFFFFFull) return DINT_ERR_ARG;
    if (freqs_dict && (freqs_dict->device != docs_dict->device || freqs_dict->kind != docs_dict->kind))
        return DINT_ERR_ARG;
    HIP_TRY(hipSetDevice(docs_dict->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // one shot: a prepared table for this call only (dint_block_table_create + dint_decode_block_table keep it)
    dint_block_table t;
    t.device = docs_dict->device;
    int st = block_table_prepare(t, d_blocks, n_blocks, index_bytes, s);
    if (st == DINT_OK) st = block_table_decode(docs_dict, freqs_dict, d_index, index_bytes, t, d_docids, d_freqs, out_capacity, s);
    (void)hipStreamSynchronize(s);  // the workspace goes away with the call
    if (t.d_ws) (void)hipFree(t.d_ws);
    return st;
}

