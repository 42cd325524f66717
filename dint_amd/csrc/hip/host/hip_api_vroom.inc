// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": the vroom decode — bundle schedule, launch_decode and its stages, dint_decode_units, prepared unit tables (single_dint::decode / multi_opt_dint::decode, vroom_env/dint_codecs.hpp:37-107, 521-619).
constexpr size_t kCounterBytes = size_t(kQueueLines) * kQueueStride * 4;  // a launch's counter lines
// The two schedule workspaces (sched_layout, split_layout: hip_stage_layout.inc) sized by the kernels' constants and placed
// in their memory.
struct placed_schedule : sched_layout {
    u32x4* d_urec = nullptr;
    uint64_t* d_cbase = nullptr;
    uint32_t *d_items = nullptr, *d_block = nullptr, *d_n_items = nullptr;
    uint8_t *d_sch = nullptr, *d_item_cnt = nullptr;
    explicit placed_schedule(size_t n) : sched_layout(n, kChunkUnits) {}
    void place(void* mem) {
        d_urec = at_byte<u32x4>(mem, urec);
        d_cbase = at_byte<uint64_t>(mem, cbase);
        d_items = at_byte<uint32_t>(mem, items);
        d_block = at_byte<uint32_t>(mem, block);
        d_n_items = at_byte<uint32_t>(mem, n_items);
        d_sch = at_byte<uint8_t>(mem, sch);
        d_item_cnt = at_byte<uint8_t>(mem, item_cnt);
    }
};
struct placed_split : split_layout {
    u32x4* d_urec = nullptr;
    uint64_t *d_cbase = nullptr, *d_end = nullptr, *d_clock = nullptr;
    uint32_t *d_left = nullptr, *d_n_left = nullptr, *d_counters = nullptr;
    explicit placed_split(size_t items) : split_layout(items, kChunkUnits, kCounterBytes) {}
    void place(void* mem) {
        d_urec = at_byte<u32x4>(mem, urec);
        d_cbase = at_byte<uint64_t>(mem, cbase);
        d_end = at_byte<uint64_t>(mem, end);
        d_left = at_byte<uint32_t>(mem, left);
        d_n_left = at_byte<uint32_t>(mem, n_left);
        d_clock = at_byte<uint64_t>(mem, clock);
        d_counters = at_byte<uint32_t>(mem, counters);
    }
};

struct deferred_launch;
// What a decode launch is asked for. Everything optional is null or 0.
struct decode_request {
    const dint_dict* dict = nullptr;
    const uint8_t* enc = nullptr;
    size_t enc_bytes = 0;
    const dint_unit* units = nullptr;
    size_t n_units = 0;
    uint32_t* out = nullptr;
    size_t out_capacity = 0;
    uint64_t* end_off = nullptr;
    hipStream_t stream = nullptr;
    // an in-index launch (any of these set: the kernels compiled for blocks, docIDs, freqs + 1; the vroom kernels carry none of it)
    uint32_t only_full = 0;
    const uint32_t* spans = nullptr;
    uint32_t plus_one = 0;
    const uint32_t* unit_base = nullptr;
    uint8_t* gaps_left = nullptr;
    const tails_args* short_blocks = nullptr;  // (a docs launch may bring its table's short blocks along: tails_phase)
    // the workspace
    sched_cache* cache = nullptr;  // a kept schedule (rebuilt under the call where it does not match); null: one of the dictionary's
    // a caller that decodes a handful of units at a time — a query's pages — does without the three schedule launches: with
    // fewer units than waves nothing is gained by sharing tiles
    size_t schedule_from = 2;
    uint32_t* zeroed_queue = nullptr;  // the caller's zeroed counters: an unscheduled launch is then the lean form
    // kQueueLines lines the caller has zeroed on this stream — a block table clears both launches' counters with ONE fill;
    // the slot still carries the launch's events
    uint32_t* own_counters = nullptr;
    deferred_launch* defer = nullptr;  // prepared, not launched: the caller launches, then finish_deferred
};

static void run_schedule_kernels(const decode_request& r, const placed_schedule& L, hipStream_t s) {
    const bool chunked = r.dict->kind == DINT_DICT_MULTI_PACKED || r.only_full != 0;
    hipLaunchKernelGGL(bundle_schedule_kernel, dim3(uint32_t(L.n_blocks)), dim3(256), 0, s, r.units, r.spans, uint64_t(r.n_units), r.enc,
                       uint64_t(r.enc_bytes), uint64_t(r.out_capacity), r.only_full, uint32_t(r.dict->kind == DINT_DICT_MULTI_PACKED),
                       uint32_t(chunked), L.d_sch, L.d_block, L.d_urec, L.d_cbase);
    if (chunked)  // (the chunked schedules: first fit)
        hipLaunchKernelGGL(bundle_pack_kernel, dim3(uint32_t((L.n_chunks + 63) / 64)), dim3(64), 0, s, L.d_urec, uint64_t(r.n_units));
    hipLaunchKernelGGL(bundle_offsets_kernel, dim3(1), dim3(1024), 0, s, L.d_block, uint32_t(L.n_blocks), L.d_n_items);
    hipLaunchKernelGGL(bundle_items_kernel, dim3(uint32_t(L.n_blocks)), dim3(256), 0, s, L.d_sch, uint64_t(r.n_units), L.d_block, L.d_items,
                       L.d_item_cnt);
}

// (Re)build the schedule of `r` in `cache` on stream `s` and remember what it was built from.
static int build_schedule(const decode_request& r, sched_cache* cache, hipStream_t s) {
    HIP_TRY(hipSetDevice(r.dict->device));
    placed_schedule L(r.n_units);
    cache->valid = false;
    if (cache->mem_bytes < L.need) {
        if (cache->d_mem) HIP_TRY(hipFree(cache->d_mem));  // (hipFree waits for the launches that read it)
        cache->d_mem = nullptr;
        cache->mem_bytes = 0;
        HIP_TRY(counted_malloc(&cache->d_mem, L.need));
        cache->mem_bytes = L.need;
    }
    L.place(cache->d_mem);
    run_schedule_kernels(r, L, s);
    HIP_TRY(hipGetLastError());
    cache->valid = true;
    cache->items_known = false;
    cache->split_ready = false;
    cache->dict = r.dict, cache->d_enc = r.enc, cache->enc_bytes = r.enc_bytes, cache->d_units = r.units, cache->n_units = r.n_units;
    cache->d_spans = r.spans, cache->out_capacity = r.out_capacity, cache->only_full = r.only_full;
    return DINT_OK;
}

// How many work items the unit queue of a kept schedule got, read back once (waits for `s`, the stream it was built on).
// None: the kernels compiled without the queue serve it.
static int read_queue_items(sched_cache& c, size_t n_units, hipStream_t s) {
    if (!c.valid || c.items_known) return DINT_OK;
    placed_schedule L(n_units);
    L.place(c.d_mem);
    uint32_t n_items = 0;
    HIP_TRY(hipMemcpyAsync(&n_items, L.d_n_items, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c.n_items = n_items;
    c.items_known = true;
    return DINT_OK;
}

// The one description of a decode launch: what launch_decode prepares — arguments, grid, queue slot, the plan — and
// launch_prepared, launch_stragglers and finish_deferred consume. A DEFERRED launch is handed to the caller prepared (slot
// taken and zeroed, schedule validated, start event recorded) to be put on the stream by it: block_table_decode's docs
// and freqs launch of an index as ONE kernel.
struct deferred_launch {
    const dint_dict* dict = nullptr;
    hipStream_t stream = nullptr;
    decode_args a{};
    tails_args short_blocks{};
    uint32_t grid = 0, slot = 0;
    uint32_t stragglers = 0;    // a kept schedule that left a few units to the queue: that many, decoded by a second, small launch
    size_t lds_bytes = 0;
    bool bundles_only = false;  // a kept schedule known to have left the unit queue empty (or to the stragglers' launch)
    bool index_launch = false, prepared = false, deferred = false;
};

static uint32_t decode_grid(const dint_dict* dd, size_t n_units) {
    const uint64_t blocks_needed = (uint64_t(n_units) + kWavesPerBlock - 1) / kWavesPerBlock;
    return uint32_t(std::min<uint64_t>(blocks_needed, std::max<uint32_t>(1, dd->compute_units) * kBlocksPerCU));
}
static size_t decode_lds_bytes(const dint_dict* dd) {
    return (size_t(dd->view.hot_words) + kClassTableWords + kWavesPerBlock * kScratchWords) * 4;
}
// The counters of a launch of `grid` workgroups in a (zeroed) counter area: unit-queue shards | the clock's line, the bundle
// path's chunk counters behind it.
static void bind_counters(decode_args& a, uint32_t* counters, uint32_t grid) {
    a.queue = counters;
    a.chunk_queue = a.queue + kQueueShards * kQueueStride;
    a.clock = reinterpret_cast<uint64_t*>(a.chunk_queue + kClockWordAt);
    a.n_shards = std::min<uint32_t>(kQueueShards, grid);
}

static void launch_prepared(const deferred_launch& d) {
    const bool multi = d.dict->kind == DINT_DICT_MULTI_PACKED;
    const dim3 grid(d.grid), block(kBlockThreads);
    if (d.index_launch && d.bundles_only)
        hipLaunchKernelGGL(multi ? decode_multi_index_bundles_kernel : decode_single_index_bundles_kernel, grid, block, d.lds_bytes, d.stream, d.a, d.short_blocks);
    else if (d.index_launch)
        hipLaunchKernelGGL(multi ? decode_multi_index_kernel : decode_single_index_kernel, grid, block, d.lds_bytes, d.stream, d.a, d.short_blocks);
    else if (multi && d.bundles_only)
        hipLaunchKernelGGL(decode_multi_bundles_kernel, grid, block, d.lds_bytes, d.stream, d.a);
    else
        hipLaunchKernelGGL(multi ? decode_multi_kernel : decode_single_kernel, grid, block, d.lds_bytes, d.stream, d.a);
}
// The few units a bundles-only launch left: a small launch of the general kernel behind it, which skips the chunks.
static void launch_stragglers(const deferred_launch& d) {
    if (!d.stragglers) return;
    decode_args b = d.a;
    b.urec = nullptr;  // (says: the unit queue only — the chunks are the first launch's)
    const uint32_t grid2 = std::min<uint32_t>(d.grid, (d.stragglers + kWavesPerBlock - 1) / kWavesPerBlock);
    b.n_shards = std::min<uint32_t>(kQueueShards, grid2);
    if (d.index_launch)
        hipLaunchKernelGGL(d.dict->kind == DINT_DICT_MULTI_PACKED ? decode_multi_index_kernel : decode_single_index_kernel, dim3(grid2),
                           dim3(kBlockThreads), d.lds_bytes, d.stream, b, tails_args{});
    else  // (a block-granular multi-dictionary unit table: the chunked schedules of the vroom kernels are its)
        hipLaunchKernelGGL(decode_multi_kernel, dim3(grid2), dim3(kBlockThreads), d.lds_bytes, d.stream, b);
}
// The cut units of a prepared multi-dictionary table, instead of its stragglers: a second launch of the bundles kernel over
// their own small schedule, the end offsets of the second halves put where the units' are, and the general kernel for
// what could not be cut.
static int launch_cut_units(const deferred_launch& d, const sched_cache& cache) {
    placed_schedule L(d.a.n_units);
    L.place(cache.d_mem);
    placed_split SL(cache.n_items);
    SL.place(cache.d_split);
    HIP_TRY(hipMemsetAsync(SL.d_counters, 0, kCounterBytes, d.stream));
    decode_args b = d.a;
    b.urec = SL.d_urec;
    b.cbase = SL.d_cbase;
    b.n_units = SL.n_sub;
    b.end_off = d.a.end_off ? SL.d_end : nullptr;
    const uint32_t grid2 = uint32_t(std::min<size_t>(d.grid, std::max<size_t>(1, (SL.n_chunks + 3) / 4)));
    bind_counters(b, SL.d_counters, grid2);
    b.clock = SL.d_clock;  // (the slot's clock word stays the main launch's)
    hipLaunchKernelGGL(decode_multi_bundles_kernel, dim3(grid2), dim3(kBlockThreads), d.lds_bytes, d.stream, b);
    if (d.a.end_off)
        hipLaunchKernelGGL(split_ends_kernel, dim3(uint32_t((cache.n_items + 255) / 256)), dim3(256), 0, d.stream, L.d_items, cache.n_items,
                           SL.d_urec, SL.d_end, d.a.end_off);
    if (cache.n_left) {
        decode_args c = d.a;
        c.urec = nullptr;  // (the unit queue only)
        c.items = SL.d_left;
        c.n_items = SL.d_n_left;
        const uint32_t grid3 = std::min<uint32_t>(d.grid, (cache.n_left + kWavesPerBlock - 1) / kWavesPerBlock);
        c.n_shards = std::min<uint32_t>(kQueueShards, grid3);
        hipLaunchKernelGGL(decode_multi_kernel, dim3(grid3), dim3(kBlockThreads), d.lds_bytes, d.stream, c);
    }
    return DINT_OK;
}
static int finish_deferred(const deferred_launch& d) {
    dint_dict* mut = const_cast<dint_dict*>(d.dict);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(mut->slot_stop[d.slot], d.stream));
    HIP_TRY(hipEventRecord(mut->slot_done[d.slot], d.stream));
    // (a deferred launch — block_table_decode's pair — comes here after launch_decode has returned and released the lock)
    std::unique_lock<std::mutex> lock(mut->launch_mutex, std::defer_lock);
    if (d.deferred) lock.lock();
    mut->slot_used[d.slot] = true;
    mut->last_slot = int(d.slot);
    return DINT_OK;
}

// ---- the stages of launch_decode, in order ---------------------------------------------------------------------------------
static deferred_launch describe_launch(const decode_request& r) {
    deferred_launch d;
    d.dict = r.dict, d.stream = r.stream;
    d.a.dict = r.dict->view;
    d.a.enc = r.enc, d.a.enc_bytes = r.enc_bytes, d.a.units = r.units, d.a.n_units = r.n_units;
    d.a.out = r.out, d.a.out_capacity = r.out_capacity, d.a.end_off = r.end_off;
    d.a.only_full = r.only_full, d.a.spans = r.spans, d.a.plus_one = r.plus_one, d.a.unit_base = r.unit_base, d.a.gaps_left = r.gaps_left;
    d.a.chunk_split_log2 = uint32_t(opt(DINT_OPT_CHUNK_SPLIT));  // (-1: by the launch's size)
    if (r.short_blocks) d.short_blocks = *r.short_blocks;
    d.grid = decode_grid(r.dict, r.n_units);
    d.lds_bytes = decode_lds_bytes(r.dict);
    d.index_launch = r.only_full != 0 || r.plus_one != 0 || r.unit_base != nullptr || r.gaps_left != nullptr;
    return d;
}

// The lean form: the caller brings the (zeroed) queue counters, nothing is timed, nothing scheduled, no slot taken — one
// API call (a query's pages: the host-side cost of a launch sequence is what a single query waits for). Nobody reads this
// launch's clock.
static int launch_decode_lean(const decode_request& r, deferred_launch& d) {
    bind_counters(d.a, r.zeroed_queue, d.grid);
    launch_prepared(d);
    HIP_TRY(hipGetLastError());
    return DINT_OK;
}

// The next queue slot of the dictionary (under launch_mutex): a reused slot's last launch waited for — normally long
// complete —, its counters bound and, unless the caller brought zeroed ones, cleared on the stream.
static int take_slot(dint_dict* dd, const decode_request& r, deferred_launch& d) {
    d.slot = dd->next_slot.fetch_add(1) % dint_dict::kQueueSlots;
    dd->launches += 1;
    if (dd->slot_used[d.slot]) HIP_TRY(hipEventSynchronize(dd->slot_done[d.slot]));
    uint32_t* const slot_counters = dd->d_queues + size_t(d.slot) * kQueueLines * kQueueStride;
    bind_counters(d.a, slot_counters, d.grid);
    // where this launch's first wave leaves its cycle count: always the slot's own line of the dictionary's counters (a block
    // table's launches bring their own ticket counters, but a table may be destroyed before somebody asks for the clock)
    uint64_t* const slot_clock = d.a.clock;
    if (r.own_counters) bind_counters(d.a, r.own_counters, d.grid);
    d.a.clock = slot_clock;
    dd->slot_clock[d.slot] = reinterpret_cast<const uint32_t*>(slot_clock);
    if (!r.own_counters) HIP_TRY(hipMemsetAsync(d.a.queue, 0, kCounterBytes, r.stream));
    return DINT_OK;
}

// The schedule of the launch, placed: the kept one — not built yet, or built for other buffers / a larger capacity:
// (re)built on this stream, and timed with the launch (the event pair spans what the call put on the stream) — or one of
// the dictionary's kSchedSlots workspaces, taken in turn, and the schedule kernels run into it.
static int choose_schedule(dint_dict* dd, const decode_request& r, uint32_t slot, placed_schedule& L, bool& start_recorded) {
    if (r.cache) {
        if (!r.cache->matches(dd, r.enc, r.enc_bytes, r.units, r.n_units, r.spans, r.out_capacity, r.only_full)) {
            HIP_TRY(hipEventRecord(dd->slot_start[slot], r.stream));
            start_recorded = true;
            const int st = build_schedule(r, r.cache, r.stream);
            if (st != DINT_OK) return st;
        }
        L.place(r.cache->d_mem);
        return DINT_OK;
    }
    const uint32_t ss = uint32_t(dd->launches % dint_dict::kSchedSlots);
    const int prev = dd->sched_user[ss];
    if (prev >= 0 && prev != int(slot) && dd->slot_used[prev]) HIP_TRY(hipEventSynchronize(dd->slot_done[prev]));
    dd->sched_user[ss] = int(slot);
    if (dd->sched_cap[ss] < L.need) {
        if (dd->d_sched[ss]) HIP_TRY(hipFree(dd->d_sched[ss]));
        dd->d_sched[ss] = nullptr;
        dd->sched_cap[ss] = 0;
        const size_t want = L.need + L.need / 4 + 4096;
        HIP_TRY(counted_malloc(&dd->d_sched[ss], want));
        dd->sched_cap[ss] = want;
    }
    L.place(dd->d_sched[ss]);
    HIP_TRY(hipEventRecord(dd->slot_start[slot], r.stream));
    start_recorded = true;
    run_schedule_kernels(r, L, r.stream);
    return DINT_OK;
}

// What a kept schedule whose queue items have been read back lets the launch do. None left to the queue (chunked
// schedules only: the vroom single-dictionary kernel's bundles ARE items of the unit queue): the kernel compiled without it.
// A FEW left — an in-index schedule: a full block of more than 504 bytes (256 postings, nearly all of them exceptions) fits
// no tile; a block-granular multi-dictionary unit table the same — the bundles through that kernel all the same, and the
// few through a small launch of the general kernel behind it (the stragglers), or as the table's cut units.
// (round 6: kMaxStragglers is a 10^8-posting index's limit — 4096 of 4 * 10^5 blocks; an index of 10^9 postings leaves
// 7.5 k, one of 5 * 10^9 38 k (multi-dictionary: 91 k / 460 k) and kept the general kernel for everything. From 2^21 blocks
// on the limit is a share of the table, as for the vroom tables: profiles/r06_inindex_scale.json)
static void plan_launch(const decode_request& r, deferred_launch& d) {
    const sched_cache& c = *r.cache;
    if (!c.items_known) return;
    const bool multi = r.dict->kind == DINT_DICT_MULTI_PACKED;
    size_t limit = 0;
    if (r.only_full != 0) limit = index_straggler_limit(r.n_units);
    else if (multi && !d.index_launch) limit = vroom_straggler_limit(r.n_units);
    if (c.n_items != 0 && c.n_items <= limit) d.stragglers = c.n_items;
    d.bundles_only = ((multi || r.only_full != 0) && c.n_items == 0) || d.stragglers != 0;
}

static int launch_decode(const decode_request& r) {
    if (!r.dict) return DINT_ERR_ARG;
    if (r.n_units == 0) return DINT_OK;
    if (!r.enc || !r.units || !r.out || r.enc_bytes < 8) return DINT_ERR_ARG;  // slots are fetched 8 bytes at a time
    HIP_TRY(hipSetDevice(r.dict->device));
    deferred_launch d = describe_launch(r);
    // tiny consecutive units are decoded several to a tile: schedule them
    const bool scheduled = r.n_units >= r.schedule_from && opt(DINT_OPT_BUNDLES) != 0;
    if (r.zeroed_queue && !scheduled) return launch_decode_lean(r, d);
    dint_dict* dd = const_cast<dint_dict*>(r.dict);
    std::lock_guard<std::mutex> lock(dd->launch_mutex);
    int st = take_slot(dd, r, d);
    if (st != DINT_OK) return st;
    bool start_recorded = false;
    if (scheduled && r.n_units < 0xFFFFFFFFull) {
        placed_schedule L(r.n_units);
        st = choose_schedule(dd, r, d.slot, L, start_recorded);
        if (st != DINT_OK) return st;
        if (r.cache) plan_launch(r, d);
        d.a.sched = L.d_sch, d.a.items = L.d_items, d.a.n_items = L.d_n_items, d.a.item_cnt = L.d_item_cnt;
        d.a.urec = L.d_urec, d.a.cbase = L.d_cbase;
    }
    if (!start_recorded) HIP_TRY(hipEventRecord(dd->slot_start[d.slot], r.stream));
    d.prepared = true;
    if (r.defer) {
        d.deferred = true;
        *r.defer = d;
        return DINT_OK;
    }
    launch_prepared(d);
    if (d.stragglers && r.cache->split_ready && !d.index_launch) {
        st = launch_cut_units(d, *r.cache);
        if (st != DINT_OK) return st;
    } else {
        launch_stragglers(d);
    }
    return finish_deferred(d);
}

int dint_decode_units(const dint_dict* dd, const uint8_t* d_enc, size_t enc_bytes, const dint_unit* d_units,
                      size_t n_units, uint32_t* d_out, size_t out_capacity, uint64_t* d_end_off, void* stream) {
    decode_request r;
    r.dict = dd, r.enc = d_enc, r.enc_bytes = enc_bytes, r.units = d_units, r.n_units = n_units;
    r.out = d_out, r.out_capacity = out_capacity, r.end_off = d_end_off, r.stream = static_cast<hipStream_t>(stream);
    return launch_decode(r);
}

struct dint_unit_table {
    const dint_dict* dict = nullptr;
    const uint8_t* d_enc = nullptr;
    size_t enc_bytes = 0;
    const dint_unit* d_units = nullptr;
    size_t n_units = 0;
    size_t out_capacity = 0;
    sched_cache sched;
    std::mutex mutex;
    // a REFINED table (refine_table): d_units / n_units above are the table's own block-granular units
    dint_unit* d_refined = nullptr;  // owned
    uint32_t* d_first = nullptr;     // owned: first[i] = the first block of the caller's unit i, n_user_units + 1 entries
    uint64_t* d_end_sub = nullptr;   // owned, made by the first decode that asks for end offsets: where every block ends
    size_t n_user_units = 0;
    // what a decode of the table asks of launch_decode, less the output (the kept schedule is built for the table's own capacity)
    decode_request request() {
        decode_request r;
        r.dict = dict, r.enc = d_enc, r.enc_bytes = enc_bytes, r.units = d_units, r.n_units = n_units;
        r.out_capacity = out_capacity, r.cache = &sched;
        return r;
    }
};

namespace {
// The blocks of a multi-dictionary table's units, found once (kernels/bundles.inc, REFINED TABLES): on success the table
// decodes its own units, one per block. Leaves the table as it came when there is nothing to gain (every unit a block
// already), a unit is longer than a lane should walk, or the walk meets something it does not understand.
constexpr uint32_t kRefineMaxInts = 1u << 17;
int refine_table(dint_unit_table* t, hipStream_t s) {
    const size_t n = t->n_units;
    HIP_TRY(hipSetDevice(t->dict->device));
    uint32_t* d_first = nullptr;
    const size_t first_words = (n + 1 + 63) / 64 * 64;  // then: max_n | bad | total, a 256-byte line
    // (no room: not refined — and the allocator's error is taken off the runtime's hands: the launches that follow poll it)
    if (counted_malloc(&d_first, (first_words + 64) * 4) != hipSuccess) {
        (void)hipGetLastError();
        return DINT_OK;
    }
    uint32_t* const d_aux = d_first + first_words;
    auto give_up = [&](int st) {
        (void)hipFree(d_first);
        return st;
    };
    uint32_t aux[3] = {0, 0, 0};
    if (!hip_ok(hipMemsetAsync(d_first, 0, (first_words + 64) * 4, s), "hipMemsetAsync")) return give_up(DINT_ERR_HIP);
    hipLaunchKernelGGL(unit_blocks_kernel, dim3(uint32_t((n + 255) / 256)), dim3(256), 0, s, t->d_units, uint64_t(n), d_first, d_aux);
    if (!hip_ok(hipGetLastError(), "unit_blocks_kernel") || !hip_ok(hipMemcpyAsync(aux, d_aux, 4, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") ||
        !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize"))
        return give_up(DINT_ERR_HIP);
    if (aux[0] <= 256 || aux[0] > kRefineMaxInts) return give_up(DINT_OK);
    hipLaunchKernelGGL(bundle_offsets_kernel, dim3(1), dim3(1024), 0, s, d_first, uint32_t(n + 1), d_aux + 2);
    if (!hip_ok(hipGetLastError(), "bundle_offsets_kernel") || !hip_ok(hipMemcpyAsync(aux, d_aux, 12, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") ||
        !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize"))
        return give_up(DINT_ERR_HIP);
    const size_t n_blocks = aux[2];
    if (n_blocks < 2 || n_blocks >= 0xFFFFFFF0ull) return give_up(DINT_OK);
    dint_unit* d_refined = nullptr;
    if (counted_malloc(&d_refined, n_blocks * sizeof(dint_unit)) != hipSuccess) {
        (void)hipGetLastError();
        return give_up(DINT_OK);
    }
    hipLaunchKernelGGL(refine_units_kernel, dim3(uint32_t((n + 63) / 64)), dim3(64), 0, s, t->d_units, uint64_t(n), d_first, t->d_enc,
                       uint64_t(t->enc_bytes), uint64_t(t->out_capacity), t->dict->view, d_refined, d_aux + 1);
    if (!hip_ok(hipGetLastError(), "refine_units_kernel") || !hip_ok(hipMemcpyAsync(aux, d_aux, 12, hipMemcpyDeviceToHost, s), "hipMemcpyAsync") ||
        !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize")) {
        (void)hipFree(d_refined);
        return give_up(DINT_ERR_HIP);
    }
    if (aux[1] != 0) {
        (void)hipFree(d_refined);
        return give_up(DINT_OK);
    }
    t->n_user_units = n;
    t->d_first = d_first;
    t->d_refined = d_refined;
    t->d_units = d_refined;
    t->n_units = n_blocks;
    return DINT_OK;
}

// (round 6) A multi-dictionary table's units that fit no tile, where they are few: cut in two records each and scheduled on
// their own (launch_cut_units decodes them). Waits for the stream.
int prepare_cut_units(dint_unit_table* t, hipStream_t s) {
    sched_cache& c = t->sched;
    if (t->dict->kind != DINT_DICT_MULTI_PACKED || c.n_items == 0 || c.n_items > vroom_straggler_limit(t->n_units) ||
        opt(DINT_OPT_SPLIT_UNITS) == 0)
        return DINT_OK;
    placed_schedule L(t->n_units);
    L.place(c.d_mem);
    placed_split SL(c.n_items);
    HIP_TRY(counted_malloc(&c.d_split, SL.need));
    SL.place(c.d_split);
    HIP_TRY(hipMemsetAsync(SL.d_n_left, 0, 256, s));
    hipLaunchKernelGGL(split_units_kernel, dim3((c.n_items + 255) / 256), dim3(256), 0, s, L.d_items, c.n_items, t->d_units, t->d_enc,
                       uint64_t(t->enc_bytes), uint64_t(t->out_capacity), t->dict->view, SL.d_urec, SL.d_cbase, SL.d_left, SL.d_n_left);
    hipLaunchKernelGGL(bundle_pack_kernel, dim3(uint32_t((SL.n_chunks + 63) / 64)), dim3(64), 0, s, SL.d_urec, uint64_t(SL.n_sub));
    HIP_TRY(hipGetLastError());
    uint32_t n_left = 0;
    HIP_TRY(hipMemcpyAsync(&n_left, SL.d_n_left, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    c.n_left = n_left;
    c.split_ready = true;
    return DINT_OK;
}
}  // namespace

int dint_unit_table_create(const dint_dict* dd, const uint8_t* d_enc, size_t enc_bytes, const dint_unit* d_units, size_t n_units,
                           size_t out_capacity, void* stream, dint_unit_table** out) {
    if (!dd || !out || (n_units && (!d_enc || !d_units || enc_bytes < 8))) return DINT_ERR_ARG;
    *out = nullptr;
    auto* t = new (std::nothrow) dint_unit_table();
    if (!t) return DINT_ERR_NOMEM;
    t->dict = dd;
    t->d_enc = d_enc;
    t->enc_bytes = enc_bytes;
    t->d_units = d_units;
    t->n_units = n_units;
    t->out_capacity = out_capacity;
    if (dd->kind == DINT_DICT_MULTI_PACKED && n_units >= 1 && n_units < 0xFFFFFFFFull && opt(DINT_OPT_BUNDLES) != 0 &&
        opt(DINT_OPT_REFINE_UNITS) != 0 && uint64_t(out_capacity) / 256 + n_units < 0xFFFFFFF0ull) {
        const int st = refine_table(t, static_cast<hipStream_t>(stream));
        if (st != DINT_OK) {
            dint_unit_table_destroy(t);
            return st;
        }
        n_units = t->n_units;  // (the table's own units, if it was refined)
    }
    if (n_units >= 2 && n_units < 0xFFFFFFFFull && !(opt(DINT_OPT_BUNDLES) == 0)) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        int st = build_schedule(t->request(), &t->sched, s);
        if (st == DINT_OK) st = read_queue_items(t->sched, n_units, s);
        if (st == DINT_OK) st = prepare_cut_units(t, s);
        if (st != DINT_OK) {
            dint_unit_table_destroy(t);
            return st;
        }
    }
    *out = t;
    return DINT_OK;
}

void dint_unit_table_destroy(dint_unit_table* t) {
    if (!t) return;
    if (t->dict) (void)hipSetDevice(t->dict->device);
    if (t->sched.d_mem) (void)hipFree(t->sched.d_mem);
    if (t->sched.d_split) (void)hipFree(t->sched.d_split);
    if (t->d_refined) (void)hipFree(t->d_refined);
    if (t->d_first) (void)hipFree(t->d_first);
    if (t->d_end_sub) (void)hipFree(t->d_end_sub);
    delete t;
}

int dint_decode_unit_table(const dint_dict* dd, dint_unit_table* t, uint32_t* d_out, size_t out_capacity, uint64_t* d_end_off,
                           void* stream) {
    if (!dd || !t || t->dict != dd || out_capacity < t->out_capacity) return DINT_ERR_ARG;
    std::lock_guard<std::mutex> lock(t->mutex);  // (the cache may be rebuilt: a dictionary created under DINT_NO_BUNDLES has none)
    uint64_t* end_arg = d_end_off;
    if (t->d_first && d_end_off) {  // a refined table: the kernels say where every BLOCK ends; the caller's units end where their last blocks do
        HIP_TRY(hipSetDevice(dd->device));
        if (!t->d_end_sub) HIP_TRY(counted_malloc(&t->d_end_sub, t->n_units * sizeof(uint64_t)));
        end_arg = t->d_end_sub;
    }
    decode_request r = t->request();
    r.out = d_out, r.out_capacity = out_capacity, r.end_off = end_arg, r.stream = static_cast<hipStream_t>(stream);
    const int st = launch_decode(r);
    if (st == DINT_OK && t->d_first && d_end_off) {
        hipLaunchKernelGGL(refined_ends_kernel, dim3(uint32_t((t->n_user_units + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                           t->d_first, uint64_t(t->n_user_units), t->d_end_sub, d_end_off);
        HIP_TRY(hipGetLastError());
    }
    return st;
}


int dint_unit_table_rank_outputs(const dint_dict* dd, dint_unit_table* t, uint32_t* const* d_outs, size_t n_outs, size_t out_capacity,
                                 void* stream, float* kernel_ms, size_t* fastest) {
    if (!dd || !t || !d_outs || n_outs == 0 || !kernel_ms) return DINT_ERR_ARG;
    for (size_t i = 0; i != n_outs; ++i)
        if (!d_outs[i]) return DINT_ERR_ARG;
    size_t best = 0;
    for (size_t i = 0; i != n_outs; ++i) {
        float ms_i = 0.f;
        for (int rep = 0; rep != 3; ++rep) {
            const int st = dint_decode_unit_table(dd, t, d_outs[i], out_capacity, nullptr, stream);
            if (st != DINT_OK) return st;
            HIP_TRY(hipStreamSynchronize(static_cast<hipStream_t>(stream)));
            float ms = 0.f;
            const int sm = dint_last_kernel_ms(dd, &ms);
            if (sm != DINT_OK) return sm;
            if (rep == 1 || (rep == 2 && ms < ms_i)) ms_i = ms;
        }
        kernel_ms[i] = ms_i;
        if (ms_i < kernel_ms[best]) best = i;
    }
    if (fastest) *fastest = best;
    return DINT_OK;
}

// ---- placement probe (round 6): the ranking of dint_unit_table_rank_outputs for the price of a SAMPLE ----------------------
// every `stride`-th run of `run` units of the caller's table, back to back (the units keep their own places in the stream
// and in the output: the sample reads and writes all over both buffers, a tenth or a fiftieth as much)
namespace {
__global__ __launch_bounds__(256) void sample_units_kernel(const dint_unit* units, uint64_t n_units, uint32_t run, uint64_t stride,
                                                           dint_unit* sample, uint64_t n_sample) {
    const uint64_t j = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (j >= n_sample) return;
    const uint64_t src = (j / run) * stride + j % run;
    sample[j] = units[src < n_units ? src : n_units - 1];
}
}  // namespace

int dint_probe_placement(const dint_dict* dd, const uint8_t* const* d_encs, size_t n_encs, size_t enc_bytes, const dint_unit* d_units,
                         size_t n_units, uint32_t* const* d_outs, size_t n_outs, size_t out_capacity, uint64_t sample_ints, void* stream,
                         float* kernel_ms) {
    if (!dd || !d_encs || !d_outs || !d_units || !kernel_ms || n_encs == 0 || n_outs == 0 || n_units == 0) return DINT_ERR_ARG;
    for (size_t i = 0; i != n_encs; ++i)
        if (!d_encs[i]) return DINT_ERR_ARG;
    for (size_t i = 0; i != n_outs; ++i)
        if (!d_outs[i]) return DINT_ERR_ARG;
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipSetDevice(dd->device));
    // runs of 4 units, evenly spread; at least 4 units a wave of the launch, at most the whole table
    const uint64_t per_unit = std::max<uint64_t>(1, uint64_t(out_capacity) / n_units);
    uint64_t want = std::max<uint64_t>(sample_ints ? sample_ints / per_unit : 0, uint64_t(16) * kWavesPerBlock * std::max<uint32_t>(1, dd->compute_units));
    want = std::min<uint64_t>(want, n_units);
    const uint32_t run = 4;
    const uint64_t n_runs = std::max<uint64_t>(1, want / run);
    const uint64_t stride = std::max<uint64_t>(run, n_units / n_runs);
    const uint64_t n_sample = std::min<uint64_t>(n_runs * run, n_units);
    dint_unit* d_sample = nullptr;
    HIP_TRY(counted_malloc(&d_sample, n_sample * sizeof(dint_unit)));
    hipLaunchKernelGGL(sample_units_kernel, dim3(uint32_t((n_sample + 255) / 256)), dim3(256), 0, s, d_units, uint64_t(n_units), run, stride,
                       d_sample, n_sample);
    int st = hip_ok(hipGetLastError(), "sample_units_kernel") ? DINT_OK : DINT_ERR_HIP;
    for (size_t i = 0; st == DINT_OK && i != n_encs; ++i)
        for (size_t j = 0; st == DINT_OK && j != n_outs; ++j) {
            float best = 0.f;
            for (int rep = 0; st == DINT_OK && rep != 4; ++rep) {
                st = dint_decode_units(dd, d_encs[i], enc_bytes, d_sample, size_t(n_sample), d_outs[j], out_capacity, nullptr, stream);
                if (st != DINT_OK) break;
                if (!hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize")) st = DINT_ERR_HIP;
                float ms = 0.f;
                if (st == DINT_OK) st = dint_last_kernel_ms(dd, &ms);
                if (rep == 1 || (rep > 1 && ms < best)) best = ms;  // (the first launch warms the schedule's workspace up)
            }
            kernel_ms[i * n_outs + j] = best;
        }
    (void)hipFree(d_sample);
    return st;
}

