// Part of dint_kernels.hpp (included from there, in order, inside namespace dint_dev): the persistent workgroup: kernel arguments as own scalars, LDS image, the sharded work queue, the five decode kernels.
// The pages of a query round (dint_query_kernels.hpp): page i = block ids[i] of the index's block table, decoded to
// docIDs at out[256 i ..). The query kernels below take their work from this instead of a unit table.
struct query_pages {
    const dint_block_ref* blocks;  // the index's block table
    const uint32_t* ids;           // page -> block
    const uint32_t* count;         // nullable: the pages in use (the device knows; the launch is sized for `bound`)
    uint64_t bound;
    uint32_t retire;               // candidate pages: the slots past a page's last posting are marked dead
    // candidate pages, term_blocks set: the first round's block-max search rides along (and_search_kernel's job, same
    // arguments) — the wave that decoded a page searches for its 256 candidates
    const uint32_t* page_query;
    const uint32_t* term_first;
    const uint32_t* term_blocks;
    const uint32_t* block_max;
    uint32_t* target;
    uint32_t* needed;
    uint32_t* rank;
    uint32_t* touched;
    uint32_t* n_touched;
    uint32_t hash_mask;            // 0, or the claim tables are hashed ones of this capacity - 1 (claim_block)
};
template <bool MULTI>
__device__ __forceinline__ void decode_query_page(const decode_args& a, const wave_ctx& c, const query_pages& qp, uint64_t page, prof_t& pf);

// Units are handed out dynamically: their cost varies a lot (a sparse list full
// of exceptions takes several times longer than a dense one of the same length),
// so a static unit -> wave map leaves most of the chip idle behind the slowest
// waves. kQueueShards counters, one per group of workgroups; a wave draws its next
// work item while it is still decoding the current one.
// The kernel arguments arrive as one 16-register scalar load; left like that, the compiler keeps (and under
// pressure spills and reloads) the whole tuple whenever one field is live — 66 v_readlane per tile in
// round 1. Passing every field through an empty asm makes each its own 32- or 64-bit scalar.
// ALL = false (the vroom single-dictionary kernel, round 6): the schedule / bundle / in-index pointers — read once per work item
// or never — are left to the compiler: 75 -> 47 spilled scalar registers, none of them in the tile loop before or after
// (profiles/r06_ab_lazy_args.txt: 1.611 against 1.617 ms per 1e9 postings). Leaving the unit table's and the output's
// pointers out as well made the allocator spill 9 VECTOR registers.
template <bool ALL = true>
__device__ __forceinline__ decode_args own_scalars(const decode_args& k) {
    decode_args a = k;
    asm volatile("" : "+s"(a.dict.tables), "+s"(a.dict.lds_image), "+s"(a.dict.descs), "+s"(a.dict.tables_bytes),
                 "+s"(a.dict.heads_base), "+s"(a.dict.tails_base), "+s"(a.dict.goff_base), "+s"(a.dict.gtable_base), "+s"(a.dict.hot_words),
                 "+s"(a.dict.first.meta_base), "+s"(a.dict.first.hot_base), "+s"(a.dict.first.hot_k));
    asm volatile("" : "+s"(a.enc), "+s"(a.enc_bytes), "+s"(a.units), "+s"(a.n_units), "+s"(a.out),
                 "+s"(a.out_capacity), "+s"(a.end_off), "+s"(a.queue), "+s"(a.n_shards), "+s"(a.only_full));
    if (ALL) asm volatile("" : "+s"(a.sched), "+s"(a.items), "+s"(a.item_cnt), "+s"(a.n_items), "+s"(a.urec), "+s"(a.cbase), "+s"(a.chunk_queue), "+s"(a.spans),
                 "+s"(a.plus_one), "+s"(a.unit_base), "+s"(a.gaps_left));
    return a;
}

// INDEX: an in-index launch (256-posting blocks: docIDs formed in the expansion, freqs + 1, full blocks only). The
// vroom kernels are compiled without any of that: the per-group branches of the expansion, and the masks the compiler
// puts on every gathered integer because the docID arithmetic might read it, are gone from their loops.
// BUNDLES_ONLY: a multi-dictionary launch whose schedule left the unit queue empty (a block-granular unit table: every
// unit fits a tile) — compiled without the unit queue and decode_unit_multi's segment loop, which is the larger half of
// the general kernel and what its register allocation is shaped by.
template <bool MULTI, bool INDEX, bool QUERY = false, bool BUNDLES_ONLY = false>
__device__ __forceinline__ void decode_kernel_body(const decode_args& kernarg, const query_pages* qp = nullptr,
                                                   const round_tail* tail = nullptr, const tails_args* short_blocks = nullptr,
                                                   uint32_t karg_at = 0) {
    decode_args a_ = own_scalars<(MULTI || INDEX || QUERY)>(kernarg);
    if (!INDEX) {
        a_.unit_base = nullptr;
        a_.gaps_left = nullptr;
        a_.plus_one = 0;
        a_.only_full = 0;
    }
    const decode_args a = a_;
    // (the first wave of the launch notes the shader clock at both ends: cycles / kernel time = the clock the kernel
    // actually ran at — boxes of one pool differ by a tenth in speed for the same binary, and this says why)
    const uint64_t clock0 = __builtin_amdgcn_s_memtime();
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    // A query's pages are dealt out, not drawn: page p is wave (p mod waves of the launch)'s. A page launch is sized for what
    // the host knows — a bound — and decodes what the round before it counted: a few hundred pages under a grid for a hundred
    // thousand. Through the unit queue every one of the 4096 waves asked its shard's counter, found it dry and went on to ask
    // the other seven — a returning atomic each, some 15 ns apiece on one address: 60 us of tickets for nothing in a launch
    // of 80 (the batch of the reference's log: two such launches a call) — and every workgroup loaded the dictionary's image
    // first. A workgroup whose first page does not exist now goes straight to the end of the launch.
    uint64_t q_work = 0;
    if (QUERY) {
        q_work = qp->bound;
        if (qp->count) q_work = uniform(*qp->count) < q_work ? uniform(*qp->count) : q_work;
    }
    const bool q_idle = QUERY && uint64_t(blockIdx.x) * kWavesPerBlock >= q_work;
    if (!q_idle) {
    // the dictionary's hot part, 16 bytes a thread and step (hot_words is a multiple of 4): five steps instead of
    // eighteen dependent round trips — nothing for a launch that decodes 10^9 integers, a third of one that decodes a
    // query's handful of pages
    // (the query kernels: all of a thread's loads in flight before the first lands in LDS — a launch of one
    // workgroup, a query's round, waits for this copy: one round trip instead of five)
    if (!QUERY) {
        for (uint32_t i = threadIdx.x; 4 * i < a.dict.hot_words; i += kBlockThreads)
            reinterpret_cast<u32x4*>(lds)[i] = reinterpret_cast<const u32x4*>(a.dict.lds_image)[i];
    } else {
        constexpr uint32_t kSteps = (kHotImageWords / 4 + kBlockThreads - 1) / kBlockThreads;
        u32x4 part[kSteps];
#pragma unroll
        for (uint32_t k = 0; k != kSteps; ++k) {
            const uint32_t i = threadIdx.x + k * kBlockThreads;
            if (4 * i < a.dict.hot_words) part[k] = reinterpret_cast<const u32x4*>(a.dict.lds_image)[i];
        }
#pragma unroll
        for (uint32_t k = 0; k != kSteps; ++k) {
            const uint32_t i = threadIdx.x + k * kBlockThreads;
            if (4 * i < a.dict.hot_words) reinterpret_cast<u32x4*>(lds)[i] = part[k];
        }
    }
    uint16_t* const cls = reinterpret_cast<uint16_t*>(lds + a.dict.hot_words);
    build_class_table(cls);
    uint32_t* const descs = lds + a.dict.hot_words + kDescWordAt;
    if (threadIdx.x < 24) descs[threadIdx.x] = MULTI ? reinterpret_cast<const uint32_t*>(a.dict.descs)[threadIdx.x] : 0u;
    const uint32_t lane = lane_id();
    const uint32_t wave = uniform(threadIdx.x / kWave);
    uint32_t* const scratch = lds + a.dict.hot_words + kClassTableWords + wave * kScratchWords;
    for (uint32_t i = lane; i < kFwWords; i += kWave) scratch[i] = 0;  // the flag words start out zero
    __syncthreads();
    wave_ctx c;
    c.lds = lds;
    c.cls = cls;
    c.descs = descs;
    c.scratch = scratch;
    c.lane = lane;
    c.rs_dict = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.dict.tables), 0, int(a.dict.tables_bytes), 0x00020000);
    c.heads_base = a.dict.heads_base;
    c.tails_base = a.dict.tails_base;
    c.goff_base = a.dict.goff_base;
    c.gtable_base = a.dict.gtable_base;
    // Work queue. Every shard — the workgroups with the same blockIdx % n_shards: one XCD under
    // round-robin placement — walks its own CONTIGUOUS part of the work items and, when that is done,
    // helps with the next shards' parts. Contiguous, because an XCD that strides over the whole
    // stream and output touches every 2 MB page of them, and past ~2 GB the translations no longer stay
    // in its TLB (the time per integer rose by a fifth); stealing, because equal counts of work items
    // are not equal work.
    const uint32_t shard = blockIdx.x % a.n_shards;  // n_shards = min(kQueueShards, gridDim.x)
    // with a schedule the queue hands out the units that are decoded on their own; the bundles follow
    const uint64_t n_work = QUERY ? q_work : a.sched ? uint64_t(uniform(*a.n_items)) : a.n_units;
    const uint64_t per_shard = (n_work + a.n_shards - 1) / a.n_shards;
    uint32_t cur = shard;
    // A draw is two steps: the ticket (one returning atomic on the shard's counter) is asked for while the
    // previous work item is still being decoded, and only looked at when that one is done — the atomic's
    // round trip (2.5k cycles per work item, 6 % of the kernel in round 1's profile) hides behind the decode.
    auto ask = [&]() -> uint32_t {
        uint32_t j = 0;
        if (lane == 0) j = __hip_atomic_fetch_add(a.queue + cur * kQueueStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return j;
    };
    auto take = [&](uint32_t ticket) -> uint64_t {  // the work item of a ticket, or ~0: nothing left anywhere
        uint32_t j = uniform(ticket);
        for (;;) {
            const uint64_t first = per_shard * cur;
            const uint64_t size = first >= n_work ? 0 : (n_work - first < per_shard ? n_work - first : per_shard);
            if (j < size) return first + j;
            // this shard is done: help the next one nobody has found dry yet (next_open_counter)
            const uint32_t next = next_open_counter(a.chunk_queue + kUnitDryWordAt, a.n_shards, cur, lane);
            if (next == ~0u) return ~0ull;
            cur = next;
            j = uniform(ask());
        }
    };
    prof_t pf;
#ifdef DINT_PROFILE
    prof_begin(pf, scratch + kScratchWords - kProfWords, lane);
#endif
    // (an in-index docs launch of a prepared table: the short blocks' tickets first — tails_phase)
    if (INDEX && !QUERY && short_blocks) {
        if (short_blocks->zero_next != nullptr && blockIdx.x == gridDim.x - 1)
            for (uint32_t i = threadIdx.x; i < short_blocks->zero_words; i += kBlockThreads) short_blocks->zero_next[i] = 0;
        SECTION(pf, 5, "short_blocks");
        tails_phase(a.enc, a.enc_bytes, *short_blocks, uint32_t(scratch - lds), lane);
        SECTION(pf, 0, "outside");
    }
    // The unit queue. In the single-dictionary kernel it hands out the bundles too, in stream order between the long
    // units: a bundle is a short, latency-bound piece of work, and with the bundles in a phase of their own — behind
    // the units, before them, or one chunk behind every eighth unit of a wave; all measured on the 1e9-posting
    // run: 2.5 %, 5 % and 3.5 % slower — too many waves wait for the same kind of round trip at the same time.
    // The multi-dictionary kernel decodes block-granular unit tables, which are bundles and nothing else: there
    // the chunks follow the (few) units on their own.
    // (Prefetching the next item's description as well — two items ahead — was measured: no gain; what a wave
    // waits for here is the vector-memory front end, not the round trip.)
    if (QUERY) {
        const uint64_t stride = uint64_t(gridDim.x) * kWavesPerBlock;
        for (uint64_t page = uint64_t(blockIdx.x) * kWavesPerBlock + wave; page < n_work; page += stride) decode_query_page<MULTI>(a, c, *qp, page, pf);
    }
    uint64_t w = BUNDLES_ONLY || QUERY ? ~0ull : take(ask());
    while (!BUNDLES_ONLY && !QUERY && w != ~0ull) {
        SECTION(pf, 14, "draw");
        uint32_t ticket = ask();
        const uint64_t uu = uniform64(!QUERY && a.sched ? uint64_t(a.items[w]) : w);
        if (QUERY) {
            decode_query_page<MULTI>(a, c, *qp, uu, pf);
        } else if (MULTI) {
            decode_unit_multi(a, c, uu, pf);
        } else {
            const uint32_t cc = uniform(a.sched ? uint32_t(a.item_cnt[w]) : 1u);
            if (__builtin_expect(cc > 1, 0)) decode_bundle_listed<false>(a, c, uu, cc, pf);
            else decode_unit_single<(!INDEX && !QUERY)>(a, c, uu, pf);  // (the vroom launches: with the stream touch)
        }
        asm volatile("" : "+v"(ticket));
        w = take(ticket);
    }
    // (an in-index launch of the single-dictionary kernel is 256-posting blocks and nothing else, like a block-granular
    // multi-dictionary table: its bundles too are found chunk by chunk, the next one's bytes requested inside the
    // current one's tile — through the unit queue every bundle paid its round trips one after the other, 0.44 ms per 10^8 postings
    // instead of 0.2x)
    if ((MULTI || (INDEX && a.only_full)) && !QUERY && a.sched && a.urec) {  // (no records: a launch for the unit queue's stragglers only)
        decode_bundle_chunks<MULTI, (MULTI && !INDEX && BUNDLES_ONLY)>(a, c, pf);
    }
#ifdef DINT_PROFILE
    prof_end(pf);
#endif
    }  // (!q_idle)
    if (blockIdx.x == 0 && threadIdx.x == 0 && (a.urec || !a.sched))  // (not the stragglers' launch: the clock is the main launch's)
    {
        // (decode_args::clock straight from the kernel-argument segment, here and nowhere else: as a field of `a` the pointer was
        // one more scalar pair live through the whole kernel — decode_single_kernel went from 0 to 1 spilled vector register.
        // `karg_at`: where this body's decode_args lies in the segment — the pair kernels' second one lies behind the first)
#if defined(__HIP_DEVICE_COMPILE__)
        typedef __attribute__((address_space(4))) const uint8_t constant_u8;
        constant_u8* kp = (constant_u8*)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(kp));
        uint64_t* const clk = *(uint64_t* __attribute__((address_space(4))) const*)(kp + karg_at + offsetof(decode_args, clock));
        *clk = __builtin_amdgcn_s_memtime() - clock0;
#else
        (void)clock0, (void)karg_at;  // (the host pass only parses this)
#endif
    }
    if (QUERY) {
        if (!tail->done) return;  // (uniform)
        // the rest of the round: by the workgroup that finishes last, with every page of the launch in memory
        // (a launch of ONE workgroup — a round of up to 16 pages, the common case of a single query — needs the
        // barrier and nothing else; an agent-scope fence writes back and invalidates this XCD's L2, microseconds each)
        __shared__ uint32_t last;
        if (gridDim.x != 1) __threadfence();  // (every wave: its pages' stores)
        __syncthreads();
        if (gridDim.x != 1) {
            if (threadIdx.x == 0) last = atomicAdd(tail->done, 1u) == gridDim.x - 1 ? 1u : 0u;
            __syncthreads();
            if (!last) return;
            __threadfence();
        }
        and_round_tail(*tail);
    }
}

#ifndef DINT_MIN_WAVES
#define DINT_MIN_WAVES 1
#endif
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_single_kernel(decode_args a) {
    decode_kernel_body<false, false>(a);
}
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_multi_kernel(decode_args a) {
    decode_kernel_body<true, false>(a);
}
// (amdgpu_num_vgpr(126): v126 / v127 are the touch loads' — decode_bundle_chunks, TOUCH)
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) __attribute__((amdgpu_num_vgpr(126))) void decode_multi_bundles_kernel(decode_args a) {
    decode_kernel_body<true, false, false, true>(a);
}
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_single_index_kernel(decode_args a, tails_args t) {
    decode_kernel_body<false, true>(a, nullptr, nullptr, &t);
}
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_multi_index_kernel(decode_args a, tails_args t) {
    decode_kernel_body<true, true>(a, nullptr, nullptr, &t);
}
// (in-index launches whose kept schedule left the unit queue empty — every full block fits a tile: all of them, in
// practice — run without the queue and the segment code, like decode_multi_bundles_kernel: no spills in the bundle loop)
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_single_index_bundles_kernel(decode_args a, tails_args t) {
    decode_kernel_body<false, true, false, true>(a, nullptr, nullptr, &t);
}
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_multi_index_bundles_kernel(decode_args a, tails_args t) {
    decode_kernel_body<true, true, false, true>(a, nullptr, nullptr, &t);
}
// The docs parts, the short blocks and the freqs parts of an index in ONE launch (dict_posting_list.hpp:284-318 is one call
// chain): every workgroup decodes docs parts until their tickets are gone, meets at a barrier, loads the freqs dictionary's
// image over the docs dictionary's and goes on with the freqs parts — two launches of persistent workgroups cannot share a CU
// (LDS), so the second waited for the first one's tail anyway; here the tail is a barrier inside a workgroup, one ticket long.
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_single_index_pair_kernel(decode_args a, decode_args b, tails_args t) {
    decode_kernel_body<false, true, false, true>(a, nullptr, nullptr, &t);
    __syncthreads();
    decode_kernel_body<false, true, false, true>(b, nullptr, nullptr, nullptr, uint32_t(sizeof(decode_args)));
}
__global__ __launch_bounds__(kBlockThreads, DINT_MIN_WAVES) void decode_multi_index_pair_kernel(decode_args a, decode_args b, tails_args t) {
    decode_kernel_body<true, true, false, true>(a, nullptr, nullptr, &t);
    __syncthreads();
    decode_kernel_body<true, true, false, true>(b, nullptr, nullptr, nullptr, uint32_t(sizeof(decode_args)));
}

