// Part of dint_kernels.hpp (included from there, in order, inside namespace dint_dev): decode_unit_single; bundles of tiny units (schedule kernels, the lane map, bundle_process, chunks), decode_unit_multi.
// A single-dictionary unit (rectangular or packed: the streams are byte-identical,
// only the dictionary source layout differed on the host) is one 16-bit segment.
// (Chaining such units like the blocks of a multi-dictionary unit — the next unit's first tiles
// requested while the current one is expanded — was measured in round 1: 5 % slower.)
// TOUCH: the segment's stream touch (kernels/segment.inc) — the vroom launches only, set at compile time (kernel_body.inc).
template <bool TOUCH>
__device__ __forceinline__ void decode_unit_single(const decode_args& a, const wave_ctx& c, uint64_t unit_index, prof_t& pf) {
    const dint_unit* up = a.units + unit_index;
    const uint64_t out_off = up->out_off;
    const uint32_t n = up->n;
    // TOUCH: the unit's byte span, for its window (dint_stream_touch.hpp) — as bundle_schedule_kernel bounds it: up to the next
    // record of the table (of a scheduled launch: the next UNIT, bundled or not), the stream's end for the last one. The next
    // record's offset is asked for here, in the same trip as this record.
    // (decode_args::spans is not looked at: only the in-index launches give spans — every caller that does sets only_full — and
    // those are compiled without the touch. Reading it here, a pointer out of the kernel-argument segment that own_scalars
    // leaves to the compiler, took decode_single_kernel from 54 to 71 spilled scalar registers and spilled a vector register.)
    constexpr bool kSpan = TOUCH && DINT_STREAM_TOUCH_LANES != 0 && DINT_STREAM_TOUCH_LINES != 0;
    const bool has_next = unit_index + 1 < a.n_units;
    uint64_t next_in_off = 0;
    if (kSpan) next_in_off = a.units[has_next ? unit_index + 1 : unit_index].in_off;
    if (n == 0 || n > kMaxUnitInts || out_off > a.out_capacity || a.out_capacity - out_off < n || (a.only_full && n != 256)) return;
    const uint64_t in_off = uniform64(up->in_off);
    uint32_t span = 0;
    if (kSpan) span = uniform(unit_stream_span(in_off, n, has_next, next_in_off, a.enc_bytes));
    chain_io ch{};
    // (in-index docs part: the flag is this wave's own — cleared here, set by the segment's first lane if the block had to be
    // left as gaps, looked at and cleared again below: nothing is left for a fix-up launch)
    volatile uint8_t* const flag = a.unit_base ? a.gaps_left + unit_index : nullptr;
    if (flag && c.lane == 0) *flag = 0;
    const uint64_t end = decode_segment<16, kRounds, kGroups, 0, TOUCH>(a, c, a.dict.first, in_off, n, a.out + out_off, ch, pf, false, false,
                                                                 a.unit_base ? a.unit_base + unit_index : nullptr,
                                                                 a.unit_base ? a.gaps_left + unit_index : nullptr, span);
    if (a.end_off && c.lane == 0) a.end_off[unit_index] = end;
    if (flag && n <= 256) {
        uint32_t left = 0;
        if (c.lane == 0) left = *flag, *flag = 0;
        if (uniform(left) != 0) gaps_to_docids_here(a.out + out_off, n, uniform(a.unit_base[unit_index]), c.lane);
    }
}

// ---- bundles of tiny units -----------------------------------------------------------------------
// Nine in ten posting lists of a Gov2-shaped collection hold at most 64 postings; as units of
// their own they are 0.2 % of the integers and a fifth of the tiles (each wave tile-step costs the
// same whether 5 or 250 of its slot positions are used). A bundle packs up to 64 consecutive tiny
// units into ONE tile: unit i takes ceil(bytes_i / 8) whole lanes, the front end runs segmented
// (per-lane slot address, carries cut at unit starts, sizes clamped at each unit's n), and because
// the units' outputs are consecutive the expansion is the ordinary one over the bundle's outputs.
constexpr uint32_t kBundleMaxInts = 256;   // a unit is bundled only if it decodes to at most this many integers
constexpr uint32_t kBundleMaxBytes = 504;  // ... and spans at most this many stream bytes (63 lanes of 8)

// Host-launched before the decode kernel: sched[i] for every unit (see decode_args::sched), and what the decode
// kernel's bundle path reads instead of the unit table — per unit one 16-byte record, per chunk of 64 units the
// stream / output offsets of its first unit:
//   urec[i] = {in_off - in0, out_off - out0, packed, 0},  packed = (n - 1) & 255 | lanes << 8 | selector << 14 | sched << 18
// (lanes: 8-byte — 8-bit slots: 4-byte — lanes of the tile the unit takes; selector: a multi-dictionary block's
// selector byte, read here so that the decode kernel does not wait for it). One workgroup per 256 units = 4 chunks.
constexpr uint32_t kChunkUnits = 64;
__global__ __launch_bounds__(256) void bundle_schedule_kernel(const dint_unit* units, const uint32_t* spans, uint64_t n_units,
                                                              const uint8_t* enc, uint64_t enc_bytes, uint64_t out_capacity,
                                                              uint32_t only_full, uint32_t multi, uint32_t chunked, uint8_t* sched,
                                                              uint32_t* block_items, u32x4* urec, uint64_t* cbase) {
    __shared__ uint32_t lanes[256], pre[256];  // lanes: the unit's lanes | its integers << 8
    __shared__ uint32_t place[256];            // first-fit launches: bundle id | first lane << 8 | member index << 16
    __shared__ uint8_t start[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = uint64_t(blockIdx.x) * 256 + tid;
    uint32_t L = 0, sel = 0;
    uint64_t in = 0, out = 0;
    uint32_t n = 0;
    if (i < n_units) {
        in = units[i].in_off;
        out = units[i].out_off;
        n = units[i].n;
    }
    // the chunk's base: its first unit (a chunk that exists has one)
    const uint64_t in0 = (uint64_t(uint32_t(__shfl(uint32_t(in >> 32), 0))) << 32) | uint32_t(__shfl(uint32_t(in), 0));
    const uint64_t out0 = (uint64_t(uint32_t(__shfl(uint32_t(out >> 32), 0))) << 32) | uint32_t(__shfl(uint32_t(out), 0));
    if (i < n_units) {
        const uint64_t nxt = spans ? in + spans[i] : (i + 1 < n_units ? units[i + 1].in_off : enc_bytes);
        // (in-index launches decode only the full blocks; the other units stay on their own and are skipped)
        // (`nxt - in0 + 16`: every byte a lane of the unit reads lies within 2^32 of the chunk's base — the lanes' slot addresses are
        // 32-bit offsets from it. Until round 6 only the unit's FIRST byte was checked: a chunk whose first unit is a short block
        // of a freqs launch has base 0 (nobody writes where a short block's docs part ends), its units carry absolute offsets,
        // and the one unit that crosses offset 2^32 of an index larger than 4 GiB wrapped: zeros from there on —
        // tools/inindex_scale.py at 5e9 postings, tests/test_gpu_index.py::test_an_index_that_straddles_4_gib)
        if (n >= 1 && n <= kBundleMaxInts && (!only_full || n == 256) && nxt > in && nxt - in <= kBundleMaxBytes &&
            nxt <= enc_bytes && out <= out_capacity && out_capacity - out >= n && in >= in0 && nxt - in0 + 16 <= 0xFFFFFFFFull && out >= out0 &&
            out - out0 < (chunked ? (1ull << 28) : (1ull << 32))) {
            if (!multi) {
                const uint32_t l = uint32_t((nxt - in + 7) >> 3);
                if (l <= kWave - 1 && in + 8ull * l <= enc_bytes) L = l;  // every lane's 8-byte load stays inside the buffer
            } else {
                // a multi unit of <= 256 integers is one block: selector byte, then 16- or 8-bit slots
                // (4 to a lane: 8 or 4 bytes); every lane still loads 8 bytes
                sel = enc[in];
                const uint32_t stride = sel >= 6 ? 4u : 8u;
                const uint32_t l = uint32_t((nxt - in - 1 + stride - 1) / stride);
                if (sel < 12 && l >= 1 && l <= kWave - 1 && in + 1 + uint64_t(stride) * l + 8 <= enc_bytes) L = l;
            }
        }
    }
    lanes[tid] = L | (n << 8);  // (n <= 256 where L != 0)
    // does this unit continue the previous one (both eligible, outputs consecutive)?
    pre[tid] = (L != 0 && tid != 0 && i < n_units && out == units[i - 1].out_off + units[i - 1].n) ? 1u : 0u;
    __syncthreads();
    // greedy packing, one thread per chunk: a bundle takes units while their lanes fit a wave (the chain through
    // in_use is the only serial part, the LDS reads are unrolled ahead of it)
    if (chunked) {
        // (the chunked launches' bundles are packed by bundle_pack_kernel, behind this kernel: here every unit
        // that fits a tile is a bundle member, the others are the unit queue's)
        start[tid] = L != 0 ? 0 : 1;
        place[tid] = 0;
    } else if ((tid & 63u) == 0) {
        uint32_t in_use = 0, ints = 0, prev_l = 0;
#pragma unroll 16
        for (uint32_t j = tid; j != tid + 64; ++j) {
            const uint32_t l = lanes[j] & 255u, m = lanes[j] >> 8;
            // (a bundle decodes to at most kMaxCap integers: one expansion batch; in-index: 8 blocks, groups = blocks)
            const bool cont = l != 0 && prev_l != 0 && pre[j] != 0 && in_use + l <= kWave && ints + m <= kMaxCap;
            start[j] = cont ? 0 : 1;
            in_use = cont ? in_use + l : l;
            ints = cont ? ints + m : m;
            prev_l = l;
        }
    }
    __syncthreads();
    uint32_t c = 0;
    if (start[tid] != 0 && i < n_units) {
        c = 1;
        if (L != 0 && !chunked)
            while (tid + c < 256 && ((tid + c) & 63u) != 0 && i + c < n_units && !start[tid + c]) ++c;
    }
    // `chunked` (the multi-dictionary kernels; the in-index launches of the single-dictionary one): the bundles are found
    // chunk by chunk (decode_bundle_chunks), a unit that fits a tile goes through the bundle path even when it has no
    // neighbour to share the tile with, and the unit queue gets the others — but not what an in-index launch skips anyway
    // (the short blocks: a ticket each for nothing). Otherwise (the single-dictionary vroom kernel) the unit queue hands
    // out everything, bundles (of two units or more) included (see decode_kernel_body).
    const bool alone = c == 1 && (L == 0 || !chunked) && !(chunked && only_full && n != 256);
    const bool item = alone || (!chunked && c > 1);
    const int n_items = __syncthreads_count(item);
    if (tid == 0) block_items[blockIdx.x] = uint32_t(n_items);
    if (i >= n_units) return;
    sched[i] = uint8_t(item ? c : 0);
    u32x4 r;
    r.x = uint32_t(in - in0);
    r.y = uint32_t(out - out0);
    r.z = ((n - 1u) & 255u) | (L << 8) | (sel << 14) | (c << 18);
    r.w = chunked ? place[tid] : 0u;
    urec[i] = r;
    if ((tid & 63u) == 0) {
        cbase[2 * (i >> 6)] = in0;
        cbase[2 * (i >> 6) + 1] = out0;
    }
}

// The multi-dictionary kernel's bundles need not be runs of consecutive units (every member's 256 outputs are an
// expansion group of their own, stored where the unit says): FIRST FIT over a few open bundles — a tile's cost
// does not depend on how full it is, and units of 15 to 40 lanes packed in order fill 51 of 64 lanes, first fit 57.
// One thread per chunk, 64 chunks to a wave (the packing of a chunk is a serial walk over its 64 units: as a loop of
// one lane per wave inside bundle_schedule_kernel it took 1.5 ms for 2e7 units; here the 64 lanes of a wave walk 64
// chunks together). Rewrites the units' records: bundle id | first lane << 8 | member index << 16 in .w, "first
// member" in the count field of .z.
__global__ __launch_bounds__(64) void bundle_pack_kernel(u32x4* urec, uint64_t n_units) {
    __shared__ uint32_t zs[64][65];  // the chunk's packed words, a row per thread (odd stride: conflict-free)
    constexpr uint32_t kOpen = DINT_FF_OPEN;
    const uint32_t tid = threadIdx.x;
    const uint64_t base = (uint64_t(blockIdx.x) * 64 + tid) * kChunkUnits;
    for (uint32_t j = 0; j != kChunkUnits; ++j) zs[tid][j] = base + j < n_units ? urec[base + j].z : 0u;
    uint32_t used[kOpen], mem[kOpen], id[kOpen], n_open = 0, next_id = 0;
#pragma unroll
    for (uint32_t k = 0; k != kOpen; ++k) used[k] = 0, mem[k] = 0, id[k] = 0;
    for (uint32_t j = 0; j != kChunkUnits; ++j) {
        const uint32_t z = zs[tid][j];
        const uint32_t l = (z >> 8) & 63u;
        uint32_t b = kOpen;
#pragma unroll
        for (uint32_t k = 0; k != kOpen; ++k)
            if (b == kOpen && k < n_open && used[k] + l <= kWave && mem[k] < 8) b = k;
        const bool fresh = b == kOpen;  // a new bundle: in a free slot, or in place of the fullest open one
        if (fresh) {
            b = n_open < kOpen ? n_open : 0u;
            if (n_open == kOpen) {
                uint32_t most = used[0];
#pragma unroll
                for (uint32_t k = 1; k != kOpen; ++k)
                    if (used[k] > most) most = used[k], b = k;
            }
        }
        uint32_t pl = 0;
#pragma unroll
        for (uint32_t k = 0; k != kOpen; ++k)
            if (k == b && l != 0) {
                if (fresh) id[k] = next_id, used[k] = 0, mem[k] = 0;
                pl = id[k] | (used[k] << 8) | (mem[k] << 16) | (mem[k] == 0 ? 1u << 31 : 0u);
                used[k] += l;
                mem[k] += 1;
            }
        if (fresh && l != 0) {
            next_id += 1;
            n_open += n_open < kOpen ? 1u : 0u;
        }
        zs[tid][j] = pl;  // (the row is this thread's own)
    }
    for (uint32_t j = 0; j != kChunkUnits; ++j) {
        const uint32_t pl = zs[tid][j];
        if (base + j < n_units && pl != 0) {  // (a member: its first-lane field or its "first" bit is set... or both are 0 only for member 0 of bundle 0 at lane 0, which has the bit)
            u32x4 r = urec[base + j];
            r.z = (r.z & ~(127u << 18)) | ((pl >> 31) << 18);
            r.w = pl & 0x7FFFFFFFu;
            urec[base + j] = r;
        }
    }
}

// ---- the units that fit no tile, SPLIT (round 6; a kept schedule of a block-granular multi-dictionary vroom table) ----------
// About one unit in a hundred of such a table is an 8-bit block of more than 252 stream bytes (many literals): it fits no
// tile, went to the unit queue, and the second launch that decoded those few through the general kernel — a unit of two
// tiles there is a chain of exposed round trips, 20 us a unit — was a TENTH of the decode (profiles/r06_kernel_stats_multi.csv:
// 1.04 of 10.0 ms for 1 % of the units). A bundle member is nothing but a record — where its slots begin, how many integers,
// how many lanes, which dictionary and slot width (the selector travels in the record: the decode kernel never reads the
// selector byte) — so such a unit is walked ONCE, when the table is prepared, and cut at a codeword boundary into two
// records that each fit a tile; the pairs form a small schedule of their own (chunks of 64 records, packed by
// bundle_pack_kernel), decoded by a second launch of the BUNDLES kernel. What cannot be cut (a half still too long, offsets
// out of a chunk's range) stays a work item of the general kernel (`left`).
// One thread per item; item j -> records 2 j and 2 j + 1; the chunk of 64 records = 32 items takes its bases from its first item.
__global__ __launch_bounds__(256) void split_units_kernel(const uint32_t* items, uint32_t n_items, const dint_unit* units, const uint8_t* enc,
                                                          uint64_t enc_bytes, uint64_t out_capacity, dict_view dv, u32x4* urec, uint64_t* cbase,
                                                          uint32_t* left_items, uint32_t* n_left) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_items) return;
    const dint_unit u = units[items[j]];
    const dint_unit u0 = units[items[j & ~31u]];
    const uint64_t in0 = u0.in_off, out0 = u0.out_off;
    if ((j & 31u) == 0) {
        cbase[2 * (j >> 5)] = in0;
        cbase[2 * (j >> 5) + 1] = out0;
    }
    u32x4 ra = {0, 0, 0, 0}, rb = {0, 0, 0, 0};
    bool ok = u.n >= 2 && u.n <= kBundleMaxInts && u.in_off < enc_bytes && u.out_off <= out_capacity && out_capacity - u.out_off >= u.n;
    if (ok) {
        const uint32_t sel = enc[u.in_off];
        ok = sel < 12;
        const bool narrow = sel >= 6;
        const uint32_t width = narrow ? 1u : 2u, stride = narrow ? 4u : 8u, max_bytes = (kWave - 1) * stride;
        const dict_desc dd = dv.descs[ok ? (narrow ? sel - 6 : sel) : 0];
        const uint64_t first = u.in_off + 1;
        uint64_t pos = first, cut = 0;
        uint32_t ints = 0, cut_ints = 0;
        while (ok && ints < u.n) {
            if (pos + 8 > enc_bytes) {
                ok = false;
                break;
            }
            const uint32_t idx = narrow ? uint32_t(enc[pos]) : uint32_t(enc[pos]) | (uint32_t(enc[pos + 1]) << 8);
            uint32_t sz = 1, step = width;
            if (idx >= 2) sz = (*reinterpret_cast<const uint32_t*>(dv.tables + dv.heads_base + 16ull * (dd.meta_base + idx)) >> 24) + 1u;
            else step = width + (idx == 1 ? 4u : 2u);
            pos += step;
            ints += sz;
            if (pos - first <= max_bytes && ints < u.n) cut = pos, cut_ints = ints;  // the first half may end here
        }
        ok = ok && cut != 0 && pos - cut <= max_bytes;
        if (ok) {
            // half A: the unit's own start (its selector byte in front of its slots); half B: one byte in front of ITS first
            // slot (a bundle member's slots begin one byte behind the record's offset: where a selector would be)
            const uint64_t in_a = u.in_off, in_b = cut - 1, out_a = u.out_off, out_b = u.out_off + cut_ints;
            const uint32_t n_a = cut_ints, n_b = u.n - cut_ints;
            const uint32_t l_a = uint32_t((cut - first + stride - 1) / stride), l_b = uint32_t((pos - cut + stride - 1) / stride);
            auto fits = [&](uint64_t in, uint32_t l, uint64_t out) {
                const uint64_t last = in + 1 + uint64_t(stride) * l + 8;  // (every lane loads 8 bytes)
                return l >= 1 && l <= kWave - 1 && last <= enc_bytes && in >= in0 && last - in0 + 16 <= 0xFFFFFFFFull && out >= out0 &&
                       out - out0 < (1ull << 28);
            };
            ok = fits(in_a, l_a, out_a) && fits(in_b, l_b, out_b);
            if (ok) {
                ra.x = uint32_t(in_a - in0), ra.y = uint32_t(out_a - out0), ra.z = ((n_a - 1u) & 255u) | (l_a << 8) | (sel << 14);
                rb.x = uint32_t(in_b - in0), rb.y = uint32_t(out_b - out0), rb.z = ((n_b - 1u) & 255u) | (l_b << 8) | (sel << 14);
            }
        }
    }
    urec[2 * j] = ra;
    urec[2 * j + 1] = rb;
    if (!ok) left_items[atomicAdd(n_left, 1u)] = items[j];
}
// ... and where a cut unit's stream ends = where its second half ends
__global__ __launch_bounds__(256) void split_ends_kernel(const uint32_t* items, uint32_t n_items, const u32x4* urec, const uint64_t* end_sub,
                                                         uint64_t* end_off) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j < n_items && ((urec[2 * j + 1].z >> 8) & 63u) != 0) end_off[items[j]] = end_sub[2 * j + 1];
}

// REFINED TABLES (round 6). A multi-dictionary unit of several blocks is decoded block after block by one wavefront — blocks carry
// no length — at half the rate of a table of blocks, whose tiles hold three blocks each (242 against 526 G ints/s on the bench
// stream). When such a table is PREPARED its blocks are found once: a lane per unit walks the unit's codewords (slot -> size,
// like split_units_kernel) and writes one unit record per block; the table then schedules and decodes the blocks.
// unit_blocks_kernel: blocks[i] = ceil(n_i / 256) (-> exclusive offsets by bundle_offsets_kernel), *max_n = the largest n.
__global__ __launch_bounds__(256) void unit_blocks_kernel(const dint_unit* units, uint64_t n_units, uint32_t* blocks, uint32_t* max_n) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    const uint32_t n = i < n_units ? units[i].n : 0u;
    if (i < n_units) blocks[i] = (n + 255u) / 256u;
    uint32_t m = n;
    for (int d = 32; d != 0; d >>= 1) {
        const uint32_t o = uint32_t(__shfl_xor(int(m), d));
        m = m > o ? m : o;
    }
    if ((threadIdx.x & 63u) == 0 && m != 0) atomicMax(max_n, m);
}
// refined[first[i] + b] = block b of unit i; *bad != 0: some unit is not what the walk understands (out of the buffer, a
// selector byte >= 12) — the caller keeps the table as it came.
__global__ __launch_bounds__(64) void refine_units_kernel(const dint_unit* units, uint64_t n_units, const uint32_t* first, const uint8_t* enc,
                                                          uint64_t enc_bytes, uint64_t out_capacity, dict_view dv, dint_unit* refined,
                                                          uint32_t* bad) {
    const uint64_t i = uint64_t(blockIdx.x) * 64 + threadIdx.x;
    if (i >= n_units) return;
    const dint_unit u = units[i];
    uint32_t k = first[i];
    bool ok = u.n != 0 && u.in_off < enc_bytes && u.out_off <= out_capacity && out_capacity - u.out_off >= u.n;
    uint64_t pos = u.in_off;
    for (uint32_t done = 0; ok && done < u.n; ++k) {
        const uint32_t bsize = u.n - done < 256u ? u.n - done : 256u;
        if (pos >= enc_bytes) {
            ok = false;
            break;
        }
        const uint32_t sel = enc[pos];
        if (sel >= 12) {
            ok = false;
            break;
        }
        dint_unit r;
        r.in_off = pos;
        r.out_off = u.out_off + done;
        r.n = bsize;
        r.list = u.list;
        refined[k] = r;
        const bool narrow = sel >= 6;
        const uint32_t width = narrow ? 1u : 2u;
        const dict_desc dd = dv.descs[narrow ? sel - 6 : sel];
        uint64_t p = pos + 1;
        for (uint32_t ints = 0; ints < bsize;) {
            if (p + width > enc_bytes) {
                ok = false;
                break;
            }
            const uint32_t idx = narrow ? uint32_t(enc[p]) : uint32_t(enc[p]) | (uint32_t(enc[p + 1]) << 8);
            uint32_t sz = 1, step = width;
            if (idx >= 2) sz = (*reinterpret_cast<const uint32_t*>(dv.tables + dv.heads_base + 16ull * (dd.meta_base + idx)) >> 24) + 1u;
            else step = width + (idx == 1 ? 4u : 2u);
            if (p + step > enc_bytes) {
                ok = false;
                break;
            }
            p += step;
            ints += sz;
        }
        pos = p;
        done += bsize;
    }
    if (!ok) atomicOr(bad, 1u);
}
// ... and where a unit of the caller's table ends = where its last block does
__global__ __launch_bounds__(256) void refined_ends_kernel(const uint32_t* first, uint64_t n_units, const uint64_t* end_sub, uint64_t* end_off) {
    const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
    if (i < n_units) end_off[i] = end_sub[first[i + 1] - 1];
}

// Work items of the unit queue = the units with sched != 0. block_items -> exclusive offsets (one
// workgroup), then every block of 256 units writes its items.
__global__ __launch_bounds__(1024) void bundle_offsets_kernel(uint32_t* block_items, uint32_t n_blocks, uint32_t* n_items) {
    __shared__ uint32_t part[1024];
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n_blocks; base += 1024) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? block_items[i] : 0;
        part[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1; d < 1024; d <<= 1) {
            const uint32_t x = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
            __syncthreads();
            part[threadIdx.x] += x;
            __syncthreads();
        }
        if (i < n_blocks) block_items[i] = carry + part[threadIdx.x] - v;
        carry += part[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_items = carry;
}

__global__ __launch_bounds__(256) void bundle_items_kernel(const uint8_t* sched, uint64_t n_units, const uint32_t* block_offsets,
                                                           uint32_t* items, uint8_t* item_cnt) {
    __shared__ uint32_t pre[256];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = uint64_t(blockIdx.x) * 256 + tid;
    const uint32_t f = i < n_units && sched[i] != 0 ? 1u : 0u;
    pre[tid] = f;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint32_t v = tid >= d ? pre[tid - d] : 0;
        __syncthreads();
        pre[tid] += v;
        __syncthreads();
    }
    if (f) {
        const uint32_t at = block_offsets[blockIdx.x] + pre[tid] - 1;
        items[at] = uint32_t(i);
        item_cnt[at] = sched[i];
    }
}

// ---- a bundle: one tile over `cnt` (2..64) consecutive tiny units starting at unit u0. MULTI: every unit is one
// block of a multi-dictionary stream — its selector byte picks the dictionary and the slot width, per unit, hence
// per lane.
// What a lane knows about its part of a bundle's tile (bundle_map), and the wave about the bundle:
struct bundle_lane {
    uint32_t par;        // its unit's n - 1 | first lane << 8 | first output (inside the bundle) << 14 | 8-bit slots << 28 | dictionary << 29
    uint32_t slot_rel;   // its first slot: byte offset from the chunk's in0
    uint32_t seg;        // its unit: member index inside the bundle (| the unit's lane in its chunk << 8: first-fit bundles)
};
struct bundle_head {     // wave-uniform ...
    uint64_t in0;        // the chunk's stream base
    uint64_t out0;       // the bundle's first output (absolute, integers); first-fit bundles: the chunk's output base
    uint32_t u0, cnt;    // first unit (first-fit bundles: the chunk's first unit), units
    uint32_t used, total;  // lanes in use (<= 64), integers (first-fit bundles: 256 per member, see below)
    // ... except, for first-fit bundles, what lane g knows about member g (= output group g): its unit's lane in the
    // chunk | its integers << 8, and its outputs' offset from the chunk's output base
    uint32_t g_unit_n, g_rel_out;
};



// Lanes and outputs of each unit by one packed scan over the units' records (one per lane, from the chunk's
// registers: unit u0 + lane is chunk lane p + lane). Registers and cross-lane operations only: it runs in the
// middle of the previous bundle's tile.
template <bool MULTI>
__device__ __forceinline__ void bundle_map(const wave_ctx& c, const u32x4& rc, uint32_t chunk, uint32_t p, uint32_t cnt, uint64_t in0,
                                           uint64_t chunk_out0, bundle_lane& bl, bundle_head& bh) {
    const uint32_t lane = c.lane;
    const bool has = lane < cnt;
    const int src = int((p + lane) & 63u);
    const uint32_t my_rel = uint32_t(__shfl(rc.x, src));
    const uint32_t my_pk = uint32_t(__shfl(rc.z, src));
    const uint32_t my_n = has ? (my_pk & 255u) + 1u : 0u;
    const uint32_t my_lanes = has ? (my_pk >> 8) & 63u : 0u;
    const uint32_t pk0 = my_n | (my_lanes << 16);
    const uint32_t inc0 = wave_inclusive_sum(pk0);
    const uint32_t my_lane0 = (inc0 - pk0) >> 16;      // first lane of this lane's unit
    bh.used = readlane(inc0, 63) >> 16;
    bh.total = readlane(inc0, 63) & 0xFFFFu;
    bh.in0 = in0;
    bh.out0 = chunk_out0 + readlane(rc.y, p);
    bh.u0 = chunk * kChunkUnits + p;
    bh.cnt = cnt;
    // lane -> unit: a bit per unit at its first lane (distinct bits: their sum is their OR), units before a lane = bits below it
    uint32_t mlo, mhi;
    if (cnt <= 12) {  // (wave-uniform; the usual bundle: a handful of blocks) the bits gathered on the scalar side
        uint64_t heads = 0;
        for (uint32_t m = 0; m != cnt; ++m) heads |= 1ull << (readlane(inc0 - pk0, m) >> 16);
        mlo = uint32_t(heads), mhi = uint32_t(heads >> 32);
    } else {
        const uint32_t hlo = has && my_lane0 < 32 ? 1u << my_lane0 : 0u, hhi = has && my_lane0 >= 32 ? 1u << (my_lane0 - 32) : 0u;
        mlo = readlane(wave_inclusive_sum(hlo), 63), mhi = readlane(wave_inclusive_sum(hhi), 63);
    }
    // (units at or before a lane, minus one = the bits of `heads >> 1` below it: lane 0 is always a head)
    const uint64_t h1 = ((uint64_t(mhi) << 32) | mlo) >> 1;
    const uint32_t seg = __builtin_amdgcn_mbcnt_hi(uint32_t(h1 >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(h1), 0u));
    const int sl_ = int(seg);
    const uint32_t seg_rel = uint32_t(__shfl(my_rel, sl_));
    const uint32_t seg_pk = uint32_t(__shfl(my_pk, sl_));
    // (first lane and first output of the unit: one value, one shuffle)
    const uint32_t seg_at = uint32_t(__shfl(inc0 - pk0, sl_));
    const uint32_t seg_lane0 = seg_at >> 16, seg_out0 = seg_at & 0xFFFFu;
    const uint32_t sel = MULTI ? (seg_pk >> 14) & 15u : 0u;
    const uint32_t narrow = sel >= 6 ? 1u : 0u;
    const uint32_t dict = narrow ? sel - 6 : sel;
    bl.par = (seg_pk & 255u) | (seg_lane0 << 8) | (seg_out0 << 14) | (narrow << 28) | (dict << 29);
    bl.slot_rel = seg_rel + (MULTI ? 1u : 0u) + (narrow ? 4u : 8u) * (lane - seg_lane0);
    bl.seg = seg;
}

// The same for a first-fit bundle: the units of the chunk whose record names bundle `b` (their first lane and member
// index come from the schedule), gathered on the scalar side — at most 8.
template <bool MULTI>
__device__ __forceinline__ void bundle_map_first_fit(const wave_ctx& c, const u32x4& rc, uint32_t chunk, uint32_t b, uint64_t in0,
                                                     uint64_t chunk_out0, bundle_lane& bl, bundle_head& bh) {
    const uint32_t lane = c.lane;
    uint64_t members = __ballot(((rc.z >> 8) & 63u) != 0 && (rc.w & 255u) == b);
    uint64_t heads = 0, units_of = 0;  // a bit at every member's first lane; member m's chunk lane in byte m
    uint32_t cnt = 0, used = 0;
    while (members != 0 && cnt != 8) {  // (in unit order = member order = lane order)
        const uint32_t u = uint32_t(__builtin_ctzll(members));
        members &= members - 1;
        const uint32_t lane0 = (readlane(rc.w, u) >> 8) & 63u;
        heads |= 1ull << lane0;
        units_of |= uint64_t(u) << (8 * cnt);
        used = lane0 + ((readlane(rc.z, u) >> 8) & 63u);
        ++cnt;
    }
    bh.used = used;
    bh.total = 256 * cnt;
    bh.in0 = in0;
    bh.out0 = chunk_out0;
    bh.u0 = chunk * kChunkUnits;
    bh.cnt = cnt;
    // (members at or before a lane, minus one = the bits of `heads >> 1` below it: lane 0 is a head)
    const uint64_t h1 = heads >> 1;
    const uint32_t seg = __builtin_amdgcn_mbcnt_hi(uint32_t(h1 >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(h1), 0u)) & 7u;
    const uint32_t unit = uint32_t(units_of >> (8 * seg)) & 63u;
    const uint32_t seg_rel = uint32_t(__shfl(rc.x, int(unit)));
    const uint32_t seg_pk = uint32_t(__shfl(rc.z, int(unit)));
    const uint32_t seg_lane0 = (uint32_t(__shfl(rc.w, int(unit))) >> 8) & 63u;
    const uint32_t sel = MULTI ? (seg_pk >> 14) & 15u : 0u;  // (single-dictionary blocks have no selector byte)
    const uint32_t narrow = sel >= 6 ? 1u : 0u;
    const uint32_t dict = narrow ? sel - 6 : sel;
    bl.par = (seg_pk & 255u) | (seg_lane0 << 8) | ((256u * seg) << 14) | (narrow << 28) | (dict << 29);
    bl.slot_rel = seg_rel + (MULTI ? 1u : 0u) + (narrow ? 4u : 8u) * (lane - seg_lane0);
    bl.seg = seg | (unit << 8);
    // lane g: member g (the shuffles with every lane enabled: a cross-lane read under `lane < cnt` finds the lanes
    // outside the branch silent)
    const uint32_t gu = uint32_t(units_of >> (8 * (lane & 7u))) & 63u;
    const uint32_t g_pk = uint32_t(__shfl(rc.z, int(gu)));
    bh.g_rel_out = uint32_t(__shfl(rc.y, int(gu)));
    bh.g_unit_n = gu | ((lane < cnt ? (g_pk & 255u) + 1u : 0u) << 8);
}

// the lane's 8 stream bytes (the schedule made sure they lie inside the buffer)
__device__ __forceinline__ uint64_t bundle_raw(const decode_args& a, const bundle_lane& bl, const bundle_head& bh, uint32_t lane) {
    uint64_t raw = 0;
    if (lane < bh.used) {
        const u32x2 r = reinterpret_cast<const u32x2_a1*>(a.enc + bh.in0 + bl.slot_rel)->v;
        raw = (uint64_t(r.y) << 32) | r.x;
    }
    return raw;
}

// COUNTED WAITS in the bundle loop (round 6). gfx950 counts vector loads and stores in one in-order counter, and what the
// compiler knows about a loaded value it has to copy at a loop's back edge is "wait for everything": the chunked bundle
// loop's `raw = raw_n` was an s_waitcnt vmcnt(0) right behind the tile's stores — every bundle waited for the acknowledgement
// of its own stores before the next one's front end began (profiles/r06_sections_multi.txt: 12.5 % of a wave's cycles between
// one bundle's last store and the next one's first instruction). The next bundle's stream bytes are therefore requested by an
// asm-issued load the compiler does not track, and the loop waits for them itself: vmcnt(k), k = the vector-memory
// instructions the tile issued BEHIND that load — its stores, one per member — which may stay in flight.
// (tools/check_inflight.py decode_multi_bundles_kernel: no compiler-generated instruction touches the load's registers
// between the load and that wait.)
#ifndef DINT_BUNDLE_COUNTED_WAIT
#define DINT_BUNDLE_COUNTED_WAIT 1
#endif
__device__ __forceinline__ uint64_t bundle_raw_async(const decode_args& a, const bundle_lane& bl, const bundle_head& bh, uint32_t lane) {
#if DINT_BUNDLE_COUNTED_WAIT && defined(__HIP_DEVICE_COMPILE__)
    // a BUFFER load, like the stores it is counted against: a global_load of the same bytes (the flat encoding) was overtaken by
    // the younger buffer stores' acknowledgements — vmcnt(k) let the wave go on before the bytes were there (1e9 postings from
    // HBM: wrong integers; an index of 1e8 postings, served from L2: none) — MUBUF loads and stores complete in issue order.
    const uint64_t room = a.enc_bytes - bh.in0;  // (the schedule made sure the chunk lies inside the buffer)
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.enc) + bh.in0, 0,
                                                                        int(room < 0xFFFFFFFFull ? uint32_t(room) : 0xFFFFFFFFu), 0x00020000);
    u32x2 r = {0u, 0u};
    if (lane < bh.used) asm volatile("buffer_load_dwordx2 %0, %1, %2, 0 offen" : "+v"(r) : "v"(bl.slot_rel), "s"(rs) : "memory");
    return (uint64_t(r.y) << 32) | r.x;
#else
    return bundle_raw(a, bl, bh, lane);
#endif
}
// ... and its wait: everything but the `younger` (wave-uniform; 0: nothing) most recent vector-memory instructions has completed
__device__ __forceinline__ void wait_all_but_youngest(uint32_t younger, uint64_t& raw) {
#if DINT_BUNDLE_COUNTED_WAIT && defined(__HIP_DEVICE_COMPILE__)
    switch (younger) {
        case 1: asm volatile("s_waitcnt vmcnt(1)" : : : "memory"); break;
        case 2: asm volatile("s_waitcnt vmcnt(2)" : : : "memory"); break;
        case 3: asm volatile("s_waitcnt vmcnt(3)" : : : "memory"); break;
        case 4: asm volatile("s_waitcnt vmcnt(4)" : : : "memory"); break;
        case 5: asm volatile("s_waitcnt vmcnt(5)" : : : "memory"); break;
        case 6: asm volatile("s_waitcnt vmcnt(6)" : : : "memory"); break;
        case 7: asm volatile("s_waitcnt vmcnt(7)" : : : "memory"); break;
        case 8: asm volatile("s_waitcnt vmcnt(8)" : : : "memory"); break;
        case 9: asm volatile("s_waitcnt vmcnt(9)" : : : "memory"); break;
        default: asm volatile("s_waitcnt vmcnt(0)" : : : "memory"); break;
    }
    // (the value is the asm's from here on — BEHIND the wait: as an operand of the wait itself the compiler copied the register
    // in front of it, before the bytes were there)
    asm volatile("" : "+v"(raw));
#else
    (void)younger, (void)raw;
#endif
}

// The tile of a mapped bundle whose stream bytes are on their way (`raw_in`). `issue_next` runs once, behind the
// tile's last wait and before its gathers and stores: the caller requests the next bundle's stream bytes there,
// so that they travel while this tile is expanded and stored.
// FF: a first-fit bundle (the chunked launches: any up to 8 units of a chunk, member m's outputs at the tile's positions [256 m, ..)
// and stored where its unit says); else a run of consecutive units with consecutive outputs (decode_bundle_listed).
// -> the vector-memory instructions issued behind issue_next (the tile's stores: one per member of a first-fit bundle), or 0:
// not known — the caller waits for everything.
template <bool MULTI, bool FF, class IssueNext>
__device__ __forceinline__ uint32_t bundle_process(const decode_args& a, const wave_ctx& c, const bundle_lane& bl, const bundle_head& bh,
                                                   uint64_t raw_in, prof_t& pf, IssueNext&& issue_next) {
    SECTION(pf, 12, "bundle_front");
    const uint32_t lane = c.lane;
    uint32_t* const scratch = c.scratch;
    const uint32_t* const lds = c.lds;
    const uint16_t* const cls = c.cls;
    const uint64_t u0 = bh.u0;
    const uint32_t cnt = bh.cnt, used = bh.used, total = bh.total;
    const uint64_t out0 = bh.out0;
    // (first-fit bundles — the multi-dictionary kernel's: the schedule checked every member's place in the output)
    if (total == 0 || (!FF && (out0 > a.out_capacity || a.out_capacity - out0 < total))) {
        issue_next();
        return 0;
    }
    const bool has = lane < cnt;
    const bool lane_used = lane < used;
    // (in-index docs parts: lane g asks for the docID base of the bundle's member g now — see docid_bases)
    docid_bases gb;
    if (a.unit_base != nullptr && has) {
        uint32_t member = uint32_t(u0) + (FF ? bh.g_unit_n & 255u : lane);
        asm volatile("" : "+v"(member));  // (one index: split into a loop-invariant `unit_base + lane` it was hoisted out of the bundle loop — and spilled)
        gb.v = a.unit_base[member];
    }
    const uint32_t seg = bl.seg & 255u;
    const uint32_t seg_unit = FF ? bl.seg >> 8 : seg;  // the lane's unit behind u0
    const uint32_t seg_n = (bl.par & 255u) + 1u;
    const uint32_t seg_lane0 = (bl.par >> 8) & 63u;
    const uint32_t seg_out0 = (bl.par >> 14) & 0x3FFFu;
    const bool seg_head = lane == seg_lane0;
    const bool narrow = MULTI && ((bl.par >> 28) & 1u) != 0;
    uint32_t hot_base = a.dict.first.hot_base, hot_k = a.dict.first.hot_k, meta_base = a.dict.first.meta_base;
    if (MULTI) {
        const uint32_t* dp = c.descs + 4 * (bl.par >> 29);
        meta_base = dp[0];
        hot_base = dp[1];
        hot_k = dp[2];
    }
    const uint64_t slot_lane = bh.in0 + bl.slot_rel;   // the lane's first slot

    // ---- slots, metadata, the cold slots' rows -----------------------------------------------------
    tile_regs cur;
    uint32_t raw_lo = 0;  // the lane's first four bytes (the next lane's: what an exception at its end spills into)
    {
        uint64_t raw = raw_in;
        asm volatile("" : "+v"(raw));  // landed
        raw_lo = uint32_t(raw);
        unpack_slots(false, raw, cur);
        if (MULTI && narrow) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) cur.s[k] = (raw_lo >> (8 * k)) & 0xFFu;
        }
    }
    // ---- classification FIRST (it needs the slots and nothing else): as in decode_segment, the carries cut at every
    // unit's first lane. The slots that are a literal's payload then ask for no head, and everything below that does not
    // depend on the metadata — the literals, the live bits — runs while the heads travel.
    SECTION(pf, 1, "b1_classify");
    tile_slots t;
    uint32_t row;
    {
        uint32_t lo = 0;
#pragma unroll
        for (uint32_t k = kSPL; k-- != 0;) lo = 3 * lo + (2u - (cur.s[k] < 2 ? cur.s[k] : 2u));
        uint32_t st_in = 0;
        const uint32_t rows_at = narrow ? kRows16 : 0u;  // the 8-bit rows follow the 16-bit ones
        for (;;) {
            row = cls[rows_at + st_in * 81 + lo];
            uint32_t prev = from_lane_below((row >> 8) & 7u);
            if (seg_head) prev = 0;
            if (__ballot(prev != st_in) == 0) break;
            st_in = prev;
        }
    }
    SECTION(pf, 3, "b2_metas_literals");
    meta_regs mr;
    head_regs hr;
    request_metas(c, hot_base, hot_k, meta_base, cur, mr, hr, row & 15u);
    const uint32_t excbits = lane_used ? (row >> 4) & 15u : 0u;
    const bool tile_exc = __ballot(excbits != 0) != 0;
    // An exception's literal: the 16 or 32 stream bits behind its marker (8-bit slots: per lane — the units of a bundle
    // differ), cut out of the lane's bytes and the next lane's; it rides into its staging cell in the second word of the
    // slot's head register, like a cold codeword's first integers (decode_segment).
    uint32_t lit[kSPL] = {0, 0, 0, 0};
    bool wide[kSPL] = {false, false, false, false};
    if (tile_exc) {
        const uint32_t raw_hi = uint32_t(raw_in >> 32);
        const uint32_t nlo = from_lane_above(raw_lo);  // (an exception's payload never leaves its unit's lanes)
        uint32_t w32[kSPL];
        w32[0] = __builtin_amdgcn_alignbit(raw_hi, raw_lo, 16);
        w32[1] = raw_hi;
        w32[2] = __builtin_amdgcn_alignbit(nlo, raw_hi, 16);
        w32[3] = nlo;
        if (MULTI) {
            const uint32_t n0 = __builtin_amdgcn_alignbit(nlo, raw_lo, 8), n1 = __builtin_amdgcn_alignbit(nlo, raw_lo, 16),
                           n2 = __builtin_amdgcn_alignbit(nlo, raw_lo, 24);
            w32[0] = narrow ? n0 : w32[0];
            w32[1] = narrow ? n1 : w32[1];
            w32[2] = narrow ? n2 : w32[2];
        }
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) {
            const uint32_t excM = uint32_t(__builtin_amdgcn_sbfe(excbits, k, 1));
            lit[k] = w32[k] & ((0u - cur.s[k]) | 0xFFFFu) & excM;  // marker 0: the 16 bits behind it; marker 1: all 32
            wide[k] = lit[k] > 0xFFFFu;
        }
    }
    take_metas(hot_k, mr, hr, cur);
    if (tile_exc) {
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) {
            const uint32_t excM = uint32_t(__builtin_amdgcn_sbfe(excbits, k, 1));
            hr.q[k].y = (hr.q[k].y & ~excM) | lit[k];
        }
    }

    SECTION(pf, 2, "b3_sizes_scans");
    // ---- sizes; positions inside each unit (one scan + the value at the unit's first lane); clamp ----
    // (a payload slot, a slot past the lane's unit: metadata masked to zero — nothing decoded, nothing taken; the two
    // exception markers look up "one integer from one staging cell", kMetaException)
    uint8_t* const lds_rw = reinterpret_cast<uint8_t*>(const_cast<uint32_t*>(lds));
    const uint32_t stage_byte0 = uint32_t(reinterpret_cast<const uint8_t*>(stage_of(scratch)) - lds_rw);
    uint32_t sz[kSPL];
    uint32_t slowb = 0;
    uint32_t liveb = lane_used ? ~row & 15u : 0u;
#pragma unroll
    for (uint32_t k = 0; k != kSPL; ++k) {
        const uint32_t lv = __builtin_amdgcn_ubfe(liveb, k, 1);
        const uint32_t m = cur.m[k] & (0u - lv);
        cur.m[k] = m;
        sz[k] = (m >> 24) + lv;
        t.need[k] = __builtin_amdgcn_ubfe(m, 20, 2);
        t.src2[k] = m & kMetaOffMask;
        slowb |= ((m >> 22) & 1u) << k;
    }
    // ---- staging cells, heads into them, tails requested — for the chunked (first-fit) bundles FIRST (round 6), before the sizes'
    // scan: the tails' round trip to L2 then runs under the scans, the end offsets and the tables instead of being waited for
    // behind them. (The cells are then allocated for every codeword header of the lanes in use: a header past its unit's last
    // integer — up to three in a unit's last lane — takes its cells and asks for its tail like the others and is simply not live
    // in the expansion.) The listed bundles of the single-dictionary vroom kernel keep the old order: the new one cost that
    // kernel a spilled vector register.
    uint32_t cell_addr[kSPL];
    uint32_t t3[kSPL];
    bool tile_big = false;
    auto take_cells = [&]() {
        const uint32_t cells = allocate_cells(t, stage_byte0, cell_addr);
        if (cells > kStageCells) {  // (as in decode_segment)
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k)
                if (t.need[k] != 0 && cell_addr[k] + 16 * t.need[k] > stage_byte0 + 16 * kStageCells) {
                    t.need[k] = 0;
                    slowb |= 1u << k;
                }
        }
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) t.src2[k] = t.need[k] != 0 ? cell_addr[k] : t.src2[k];
    };
    auto heads_and_tails = [&]() {
        // the heads into their cells; the tails of the large ones requested (they land behind the flag/delta phase: decode_segment)
        heads_into_cells<!MULTI>(lds_rw, t, hr, wide);
        tile_big = __ballot((t.need[0] | t.need[1] | t.need[2] | t.need[3]) > 1u) != 0;  // some codeword needs its tail
        if (tile_big) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) {
                const uint32_t tail = c.tails_base + 32 * (meta_base + cur.s[k]);
                if (t.need[k] > 1u) hr.q[k] = __builtin_amdgcn_raw_buffer_load_b128(c.rs_dict, tail, 0, 0);
                if (t.need[k] > 2u) t3[k] = __builtin_amdgcn_raw_buffer_load_b32(c.rs_dict, tail + 16, 0, 0);
            }
        }
    };
    if (FF) {
        take_cells();
        heads_and_tails();
    }
    // ---- positions inside each unit (one scan + the value at the unit's first lane); clamp ----
    t.off[0] = 0;
#pragma unroll
    for (uint32_t k = 1; k != kSPL; ++k) t.off[k] = t.off[k - 1] + sz[k - 1];
    const uint32_t raw_sum = t.off[kSPL - 1] + sz[kSPL - 1];
    const uint32_t inc1 = wave_inclusive_sum(raw_sum);
    // (the read is unconditional: ds_bpermute returns nothing from lanes that do not take part)
    const uint32_t inc1_before = uint32_t(__shfl(inc1, int(seg_lane0 + 63u) & 63));
    const uint32_t before_seg = seg_lane0 == 0 ? 0u : inc1_before;
    const uint32_t p0 = inc1 - raw_sum - before_seg;  // position of the lane's first codeword inside its unit
    uint32_t nlive = 0, lsum = 0, lb = 0;
#pragma unroll
    for (uint32_t k = 0; k != kSPL; ++k) {
        const uint32_t pos = p0 + t.off[k];
        const bool act = ((liveb >> k) & 1u) != 0 && pos < seg_n;
        const uint32_t room = seg_n - pos;
        lb |= (act ? 1u : 0u) << k;
        nlive += act ? 1u : 0u;
        lsum += act ? (sz[k] < room ? sz[k] : room) : 0u;
        if (!FF && !act) t.need[k] = 0;
    }
    liveb = lb;
    t.row = row;
    t.liveb = liveb;
    t.lsum = lsum;
    t.nlive = nlive;
    t.obase = seg_out0 + p0;
    t.rbase = wave_inclusive_sum(nlive) - nlive;
    t.total = total;
    slowb &= liveb;
    if (!FF) take_cells();
    const bool tile_wide = tile_exc && __ballot(wide[0] || wide[1] || wide[2] || wide[3]) != 0;
    const bool tile_slow = __ballot(slowb != 0) != 0;

    SECTION(pf, 11, "b4_cells_tails");
    // where each unit's stream ends: after its last live codeword (and that one's payload). That codeword
    // sits in the unit's highest lane that has a live one: the next such lane belongs to another unit.
    if (a.end_off) {
        uint32_t last_end = 0;  // slots from the lane's first to the end of its last live codeword
        // (branch-free: as `if`s the compiler made four nests of exec-mask branches of this — 28 saveexec / 19 branches a bundle)
        const uint32_t pay_shift = narrow ? 1u : 0u;  // an exception marker s (0 / 1) owns s + 1 payload slots (8-bit slots: 2 s + 2)
        if (FF) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) {
                const uint32_t lvM = uint32_t(__builtin_amdgcn_sbfe(liveb, k, 1));    // all ones: slot k is a live codeword
                const uint32_t exM = uint32_t(__builtin_amdgcn_sbfe(excbits, k, 1));  // ... an exception marker
                const uint32_t e = k + 1u + (((cur.s[k] + 1u) << pay_shift) & exM);
                last_end = (e & lvM) | (last_end & ~lvM);
            }
        } else {  // (the single-dictionary vroom kernel's listed bundles: as it was — the rewrite cost that kernel a spilled register)
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k)
                if ((liveb >> k) & 1u)
                    last_end = k + 1 + (((excbits >> k) & 1u) ? (narrow ? 2 * cur.s[k] + 2u : cur.s[k] + 1u) : 0u);
        }
        const uint64_t havers = __ballot(last_end != 0);
        const uint64_t above = lane == 63 ? 0ull : havers & ~((2ull << lane) - 1ull);
        const uint32_t next_lane = above ? uint32_t(__builtin_ctzll(above)) : lane;
        const uint32_t next_seg = uint32_t(__shfl(seg, int(next_lane)));  // (unconditional: every lane takes part)
        if (last_end != 0 && (above == 0 || next_seg != seg))
            a.end_off[u0 + seg_unit] = slot_lane + (narrow ? 1ull : 2ull) * last_end;
    }

    uint32_t* const out = a.out + out0;
    uint32_t* const out_u = reinterpret_cast<uint32_t*>(uniform64(reinterpret_cast<uint64_t>(out)));
    // (first-fit bundles: rs_out is the slow path's only — everything from the chunk's output base on, see store_shift)
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out_u, 0, FF ? 0x7FFFFFFC : int(total * 4), 0x00020000);
    group_out go{out_u, bh.g_unit_n, bh.g_rel_out};
    if (!FF) heads_and_tails();
    // (in-index docs parts: every unit of the bundle is a 256-posting block, so group g of the expansion is unit
    // u0 + g; a slow codeword anywhere leaves the whole bundle as gaps for the flagged fix-up)
    const bool as_docids = a.unit_base != nullptr && !tile_slow && total <= kMaxCap;
    // (a bundle is one batch by construction: the schedule packs at most kMaxCap integers into one)
#ifndef DINT_BUNDLE_GROUPS
#define DINT_BUNDLE_GROUPS DINT_GROUPS
#endif
    gb.on = as_docids;
    expand_tile<8 / DINT_BUNDLE_GROUPS, DINT_BUNDLE_GROUPS, true>(t, false, tile_wide, a.plus_one, gb, 0u, lds, scratch, rs_out, lane, pf, [&]() {
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) asm volatile("" : "+v"(hr.q[k]), "+v"(t3[k]));
        if (a.unit_base != nullptr) asm volatile("" : "+v"(gb.v));  // landed
        if (tile_big) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) {
                if (t.need[k] > 1u) *reinterpret_cast<u32x4*>(lds_rw + t.src2[k] + 12) = hr.q[k];
                if (t.need[k] > 2u) *reinterpret_cast<uint32_t*>(lds_rw + t.src2[k] + 28) = t3[k];
            }
        }
        wave_lds_fence();
        SECTION(pf, 15, "b5_next_bundle");
        issue_next();
    }, FF ? &go : nullptr);
    if (tile_slow) {
        // (positions in slow_stores are relative to the bundle; a unit's clamp is what `room` must be)
        const uint8_t* const my_slots = a.enc + slot_lane;
        // first-fit bundles: the lane's unit's outputs begin at its own offset, not at the tile's position 256 * member
        const uint32_t shift = FF ? uint32_t(__shfl(bh.g_rel_out, int(seg))) - seg_out0 : 0u;
        slow_stores(MULTI && narrow, c, t, slowb, a.plus_one, 0u, seg_out0 + seg_n, my_slots, hot_base, hot_k, meta_base, rs_out, shift);
    }
    // (in-index docs parts the expansion had to leave as gaps — a slow codeword in the bundle: next to none — become docIDs
    // here, member by member; only first-fit bundles carry docID bases: the in-index launches' are)
    const bool fixed_up = FF && a.unit_base != nullptr && !as_docids;
    if (fixed_up) {
        for (uint32_t g = 0; g != cnt; ++g)
            gaps_to_docids_here(go.base + readlane(go.rel_out, g), readlane(go.unit_n, g) >> 8, readlane(gb.v, g), lane);
    }
    SECTION(pf, 13, "epilogue");
    // (a first-fit bundle's expansion is one 16-byte store instruction per member: group_out)
    return FF && !tile_slow && !fixed_up && cnt <= 8 ? cnt : 0u;
}

// The bundle path of a launch: chunks of 64 units are drawn from one counter; a chunk's records arrive in ONE load
// (requested a chunk ahead), its bundles — the lanes whose record says "leads c units" — are mapped from
// registers, and every bundle's stream bytes are requested while the bundle before it is expanded. Round 2's
// first version walked a list of bundles instead and paid, per bundle of some 900 integers, one full memory
// round trip each for the list entry, the units' descriptors, their selector bytes and their slots: 36 % of the
// multi-dictionary kernel's time, and 19 % more waiting for the queue ticket behind the previous bundle's stores.
// One bundle on its own, named by its first unit (the single-dictionary kernel's unit queue hands bundles out between
// the long units: see decode_kernel_body): its chunk's records, then as below.
template <bool MULTI>
__device__ __forceinline__ void decode_bundle_listed(const decode_args& a, const wave_ctx& c, uint64_t u0, uint32_t cnt, prof_t& pf) {
    const uint32_t lane = c.lane;
    const uint32_t ch = uint32_t(u0 / kChunkUnits), p = uint32_t(u0 % kChunkUnits);
    const uint64_t i = uint64_t(ch) * kChunkUnits + lane;
    u32x4 rc = {0, 0, 0, 0};
    if (i < a.n_units) rc = a.urec[i];
    const u32x4 cb = *reinterpret_cast<const u32x4*>(a.cbase + 2 * uint64_t(ch));
    const uint64_t in0 = (uint64_t(uniform(cb.y)) << 32) | uniform(cb.x), out0 = (uint64_t(uniform(cb.w)) << 32) | uniform(cb.z);
    bundle_lane bl;
    bundle_head bh;
    bundle_map<MULTI>(c, rc, ch, p, cnt, in0, out0, bl, bh);
    const uint64_t raw = bundle_raw(a, bl, bh, lane);
    bundle_process<MULTI, false>(a, c, bl, bh, raw, pf, []() {});
}

// The chunks' tickets come from kChunkShards counters, a 128-byte line each: the workgroups of one XCD (blockIdx % 8) share
// four of them, every counter owns a CONTIGUOUS range of the tickets (an XCD walks its own part of the stream and
// output, like the unit queue's shards) and a wave whose counter has run dry helps with the next one's range. ONE counter
// — rounds 2 to 4 — is a returning device-scope atomic on one address, and the chip does about one such every 15 ns:
// the 3.05e5 chunks of the 5e9-integer multi-dictionary run were 4.6 ms of atomics in a 10.4 ms kernel, and tickets
// finer than a chunk (below) made the counter what the launch waited for (4e8 integers: 1.13 -> 1.52 ms).
struct chunk_queue_state {
    uint32_t cur, n_counters, per, n_tickets;
};
__device__ __forceinline__ uint32_t chunk_ask(const decode_args& a, const chunk_queue_state& q, uint32_t lane) {
    uint32_t j = 0;
    if (lane == 0) j = __hip_atomic_fetch_add(a.chunk_queue + kChunkCounterLineAt * kQueueStride + q.cur * kQueueStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return j;
}
// the global ticket of what a counter handed out, or ~0u: nothing left anywhere.
// A wave whose counter has run dry says so in a word all waves of the launch read (a bit per counter, in the clock's line)
// and goes on to a counter nobody has found dry yet. Until round 5 it asked the counters one after the other: at the end of
// a launch every one of the 4096 waves swept all 32 — 131 k returning atomics on 32 addresses, one every ~15 ns per
// address: 60 us in which nothing was decoded, at the end of each phase of a 0.4 ms in-index launch (the same sweep over
// the unit queue's shards was most of a query round's page launch). The word is read by a load — loads of one address do
// not queue the way its read-modify-writes do — and written (no value back) only by the waves that find a counter dry
// before anybody has said so.
__device__ __forceinline__ uint32_t next_open_counter(uint32_t* dry, uint32_t n_counters, uint32_t cur, uint32_t lane) {
    uint32_t m = 0;
    if (lane == 0) m = __hip_atomic_load(dry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    m = uniform(m);
    const uint32_t bit = 1u << cur;
    if ((m & bit) == 0 && lane == 0) (void)__hip_atomic_fetch_or(dry, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t open = ~(m | bit) & (n_counters >= 32 ? ~0u : (1u << n_counters) - 1u);
    if (open == 0) return ~0u;
    const uint32_t above = cur >= 31 ? 0u : open & ~((2u << cur) - 1u);  // the next one, round the ring
    return uint32_t(__builtin_ctz(above ? above : open));
}
__device__ __forceinline__ uint32_t chunk_take(const decode_args& a, chunk_queue_state& q, uint32_t drawn, uint32_t lane) {
    uint32_t j = uniform(drawn);
    for (;;) {
        const uint32_t first = q.per * q.cur;
        const uint32_t size = first >= q.n_tickets ? 0u : (q.n_tickets - first < q.per ? q.n_tickets - first : q.per);
        if (j < size) return first + j;
        const uint32_t next = next_open_counter(a.chunk_queue + kChunkDryWordAt, q.n_counters, q.cur, lane);
        if (next == ~0u) return ~0u;
        q.cur = next;
        j = uniform(chunk_ask(a, q, lane));
    }
}
// TOUCH (round 6; the vroom launches of a block-granular table): when a wave takes a new chunk, every unit's lane touches the
// first two 128-byte lines of the unit's stream bytes — the bundles' own loads, a tile ahead each, then find the lines in L2
// instead of HBM (a tile is ~2000 cycles, an HBM trip under this load more): -3.9 % at 1e9 postings
// (profiles/r06_ab_bundle_loop.txt). Not for the in-index launches: +2-3 % at 1e8 postings, where the index is cache-resident
// anyway and the two more live registers spill in the pair kernels.
template <bool MULTI, bool TOUCH = false>
__device__ __forceinline__ void decode_bundle_chunks(const decode_args& a, const wave_ctx& c, prof_t& pf) {
    const uint32_t lane = c.lane;
    const uint32_t n_chunks = uint32_t((a.n_units + kChunkUnits - 1) / kChunkUnits);
    // A ticket is a PART of a chunk: the bundles led by the units of one 1/S of the chunk's lanes (a bundle does not cross
    // chunks; its leader's lane says whose it is). A chunk of 256-integer units is ~25 tiles, 0.1-0.2 ms of a wave: an
    // in-index decode of 10^8 postings is 1.6 chunks to a wave, and with whole chunks the launch lasted as long as the waves
    // that drew two (0.33 ms of a kernel whose waves averaged 0.24). The price of a part: the chunk's records are loaded by
    // every wave that draws one, a round trip nothing hides. Measured (tools/split_sweep.py, multi_packed_dint, 256-integer
    // units, ms per launch at S = 1 / 2 / 4 / 8 / 16): 4e8 integers 0.921 / - / 0.822 / 0.861 / 0.922; 2e9: 4.147 / 4.081 /
    // 4.088 / 4.194 / -. Whole chunks first and parts at the end of every counter's range (guided) was slower than parts
    // throughout (4e8: 1.09 against 1.02 ms with the schedule kernels; in-index 0.475 against 0.442).
    const uint32_t n_waves = gridDim.x * kWavesPerBlock;
    // (every part re-reads its chunk's records and maps its first bundle with nothing ahead of it: +10 % vector instructions
    // per integer at a quarter of a chunk per ticket — worth it while a wave draws few chunks, not at 74 chunks to a wave)
    const uint32_t split_auto = n_chunks >= 64 * n_waves ? 0u : n_chunks >= 16 * n_waves ? 1u : n_chunks >= 4 * n_waves ? 2u : n_chunks >= n_waves ? 3u : 4u;
    const uint32_t split_log2 = a.chunk_split_log2 <= 4u ? a.chunk_split_log2 : split_auto;  // (dint_set_option(DINT_OPT_CHUNK_SPLIT): a measurement's)
    const uint32_t part_lanes = kChunkUnits >> split_log2;
    auto part_mask = [&](uint32_t ticket) -> uint64_t {
        if (split_log2 == 0) return ~0ull;
        const uint32_t part = ticket & ((1u << split_log2) - 1u);
        return ((1ull << part_lanes) - 1ull) << (part * part_lanes);
    };
    chunk_queue_state q;
    q.n_tickets = n_chunks << split_log2;  // (n_chunks < 2^26: n_units < 2^32)
    q.n_counters = kChunkShards;
    q.per = (q.n_tickets + q.n_counters - 1) / q.n_counters;
    q.cur = ((blockIdx.x % kQueueShards) * (kChunkShards / kQueueShards) + (uniform(threadIdx.x / kWave) % (kChunkShards / kQueueShards))) % q.n_counters;
    auto ask = [&]() -> uint32_t { return chunk_ask(a, q, lane); };
    auto records = [&](uint32_t chunk) -> u32x4 {
        const uint64_t i = uint64_t(chunk) * kChunkUnits + lane;
        u32x4 r = {0, 0, 0, 0};
        if (i < a.n_units) r = a.urec[i];
        return r;
    };
    auto bases = [&](uint32_t chunk) -> u32x4 {  // (every lane the same 16 bytes: one request)
        return *reinterpret_cast<const u32x4*>(a.cbase + 2 * uint64_t(chunk));
    };
    auto leaders = [&](const u32x4& r) -> uint64_t { return __ballot(((r.z >> 18) & 127u) != 0 && ((r.z >> 8) & 63u) != 0); };
    // chunk `ch` (records rc, bases in0 / out0, bundle leaders left: lm); the next chunk's ticket in flight. (The next
    // chunk's records are NOT requested ahead: eight more registers live through every tile of the chunk cost more
    // — as spills, each reload a wait for everything in flight — than one exposed round trip per chunk.)
    uint32_t tk = ask();  // the wave's next ticket, as its counter drew it: in flight
    uint32_t ch = chunk_take(a, q, tk, lane);
    if (ch == ~0u) return;
    uint64_t mine = part_mask(ch);
    ch >>= split_log2;
    u32x4 rc = records(ch);
    uint64_t in0, out0;
    {
        const u32x4 cb = bases(ch);
        in0 = (uint64_t(uniform(cb.y)) << 32) | uniform(cb.x);
        out0 = (uint64_t(uniform(cb.w)) << 32) | uniform(cb.z);
    }
    tk = ask();
    uint64_t lm = leaders(rc) & mine;
    // -> the next bundle: (chunk registers current, p); false: nothing left
    uint32_t p = 0;
    auto touch_chunk = [&]() {
#if defined(__HIP_DEVICE_COMPILE__)
        if (!TOUCH) return;
        // Nothing reads what these loads return, and nothing may live where they land until they have: their destinations are
        // v126 / v127, which the kernel that sets TOUCH keeps out of the register allocator's hands (amdgpu_num_vgpr(126),
        // kernel_body.inc) — as variables of the loop the compiler moved them from register to register, and a register it had
        // moved one out of was free for another value while the load was still on its way (tools/check_inflight.py).
        const uint64_t room = a.enc_bytes - in0;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(a.enc) + in0, 0,
                                                                            int(room < 0xFFFFFFFFull ? uint32_t(room) : 0xFFFFFFFFu), 0x00020000);
        const uint32_t lanes_ = (rc.z >> 8) & 63u;
        if (lanes_ != 0 && ((mine >> lane) & 1ull) != 0) {
            asm volatile("buffer_load_dword v126, %0, %1, 0 offen" : : "v"(rc.x & ~3u), "s"(rs) : "memory", "v126");
            if (lanes_ > 16) asm volatile("buffer_load_dword v127, %0, %1, 0 offen offset:128" : : "v"(rc.x & ~3u), "s"(rs) : "memory", "v127");
        }
#endif
    };
    auto advance = [&]() -> bool {
        while (lm == 0) {
            const uint32_t t2 = chunk_take(a, q, tk, lane);
            if (t2 == ~0u) return false;
            mine = part_mask(t2);
            ch = t2 >> split_log2;
            rc = records(ch);
            const u32x4 cb = bases(ch);
            in0 = (uint64_t(uniform(cb.y)) << 32) | uniform(cb.x);
            out0 = (uint64_t(uniform(cb.w)) << 32) | uniform(cb.z);
            tk = ask();
            lm = leaders(rc) & mine;
            touch_chunk();
        }
        p = uint32_t(__builtin_ctzll(lm));
        lm &= lm - 1;
        return true;
    };
    auto map_here = [&](bundle_lane& l, bundle_head& h) {
        bundle_map_first_fit<MULTI>(c, rc, ch, readlane(rc.w, p) & 255u, in0, out0, l, h);  // (the chunked schedules are first-fit ones)
    };
    if (!advance()) return;
    bundle_lane bl;
    bundle_head bh;
    map_here(bl, bh);
    uint64_t raw = bundle_raw_async(a, bl, bh, lane);
#ifndef DINT_BUNDLE_RAW_AHEAD
#define DINT_BUNDLE_RAW_AHEAD 1
#endif
#if DINT_BUNDLE_RAW_AHEAD == 2
    // The stream bytes of a bundle are requested TWO bundles ahead (round 6): one bundle ahead — a tile's expansion and stores,
    // some 2000 cycles — the load was still on its way from HBM when the loop came round (profiles/r06_sections_multi.txt: 12.5 %
    // of a wave's cycles at the loop's end), and with the counted wait it is the load, not the stores behind it, that is waited for.
    // `n1`: the bundle decoded next (mapped, its bytes in flight since the tile before this one); `n2`: the one after, found,
    // mapped and requested inside this tile. The wait at the loop's end is for n1's bytes: behind them in the counter are n2's
    // request and this tile's stores.
    bundle_lane bl1;
    bundle_head bh1;
    uint64_t raw1 = 0;
    bool have1 = advance();
    if (have1) {
        map_here(bl1, bh1);
        raw1 = bundle_raw_async(a, bl1, bh1, lane);
    }
    wait_all_but_youngest(have1 ? 1u : 0u, raw);
    for (;;) {
        bundle_lane bl2;
        bundle_head bh2;
        bool have2 = false;
        uint64_t raw2 = 0;
        const uint32_t stores = bundle_process<MULTI, true>(a, c, bl, bh, raw, pf, [&]() {
            have2 = have1 && advance();
            if (have2) {
                map_here(bl2, bh2);
                raw2 = bundle_raw_async(a, bl2, bh2, lane);
            }
        });
        if (!have1) break;
        // (stores == 0: the tile issued vector-memory instructions of its own count — the slow path — wait for everything)
        wait_all_but_youngest(stores != 0 ? stores + (have2 ? 1u : 0u) : 0u, raw1);
        bl = bl1, bh = bh1, raw = raw1;
        bl1 = bl2, bh1 = bh2, raw1 = raw2;
        have1 = have2;
    }
#else
    wait_all_but_youngest(0, raw);
    for (;;) {
        // the bundle after this one is found, mapped and its bytes requested in the middle of this one's tile: behind
        // its last wait (what that needs from memory — a chunk's records, spilled registers — is no wait for stores
        // there: this tile's have not been issued), before its gathers and stores
        bundle_lane bl_n;
        bundle_head bh_n;
        bool have_n = false;
        uint64_t raw_n = 0;
        const uint32_t younger = bundle_process<MULTI, true>(a, c, bl, bh, raw, pf, [&]() {
            have_n = advance();
            if (have_n) {
                map_here(bl_n, bh_n);
                raw_n = bundle_raw_async(a, bl_n, bh_n, lane);
            }
        });
        if (!have_n) break;
        wait_all_but_youngest(younger, raw_n);  // the next bundle's bytes are here; this tile's stores may still be on their way
        bl = bl_n;
        bh = bh_n;
        raw = raw_n;
    }
#endif
}

// A multi-dictionary unit: blocks of 256 integers (the last one shorter), each opened
// by a selector byte: < 6 -> 16-bit codewords against dictionary `selector`, else 8-bit
// codewords against dictionary `selector - 6` (vroom_env/dint_codecs.hpp:521-619).
// Blocks carry no length, so they are decoded one after the other.
__device__ __forceinline__ void decode_unit_multi(const decode_args& a, const wave_ctx& c, uint64_t unit_index, prof_t& pf) {
    const uint32_t lane = c.lane;
    const dint_unit* up = a.units + unit_index;
    const uint64_t out_off = up->out_off;
    const uint32_t n = up->n;
    if (n == 0 || n > kMaxUnitInts || out_off > a.out_capacity || a.out_capacity - out_off < n || (a.only_full && n != 256)) return;
    uint64_t pos = up->in_off;
    chain_io ch{};
    // (in-index docs part, a unit = one block: see decode_unit_single)
    volatile uint8_t* const flag = a.unit_base ? a.gaps_left + unit_index : nullptr;
    if (flag && lane == 0) *flag = 0;
    for (uint32_t done = 0; done < n;) {
        const uint32_t bsize = n - done < 256u ? n - done : 256u;
        pos = uniform64(pos);
        // chained unless the block sits in the last kChainBytes of the buffer
        const bool chained = pos <= a.enc_bytes && a.enc_bytes - pos >= 1 + kChainBytes;
        if (chained && !ch.valid) chain_request(a.enc, pos, lane, ch);  // first block of the unit
        uint32_t sel;
        if (chained) {
            sel = uniform(ch.sel) & 0xFFu;
        } else {
            const uint64_t sp = pos < a.enc_bytes ? pos : a.enc_bytes - 1;
            sel = uniform(a.enc[sp]);
        }
        const bool narrow = sel >= 6;
        const uint32_t d = (narrow ? sel - 6 : sel) % 6;
        dict_desc dd;
        dd.meta_base = uniform(c.descs[4 * d]);
        dd.hot_base = uniform(c.descs[4 * d + 1]);
        dd.hot_k = uniform(c.descs[4 * d + 2]);
        dd.pad = 0;
        uint32_t* const out = a.out + out_off + done;
        ch.more = done + bsize < n;
        pos = decode_segment<0, 1, 1, -1>(a, c, dd, pos + 1, bsize, out, ch, pf, narrow, chained,
                                          a.unit_base ? a.unit_base + unit_index : nullptr,
                                          a.unit_base ? a.gaps_left + unit_index : nullptr);
        done += bsize;
    }
    if (a.end_off && lane == 0) a.end_off[unit_index] = pos;
    if (flag && n <= 256) {
        uint32_t left = 0;
        if (lane == 0) left = *flag, *flag = 0;
        if (uniform(left) != 0) gaps_to_docids_here(a.out + out_off, n, uniform(a.unit_base[unit_index]), lane);
    }
}

