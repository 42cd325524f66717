// Part of dint_kernels.hpp (included from there, in order, inside namespace dint_dev): device views of a dictionary and of a launch (dict_view, decode_args), wave-level helpers (DPP scans, lane moves, LDS fence), a lane's slots from an arbitrary byte address, the slot classification table, section marks.
// One dictionary of the (possibly multi-) dictionary file.
struct dict_desc {
    uint32_t meta_base;    // first slot of this dictionary in gmeta / the row table
    uint32_t hot_base;     // LDS word offset of its hot meta table
    uint32_t hot_k;        // codewords < hot_k have meta + payload in the LDS image
    uint32_t pad;
};

// Device view of a dictionary file (layout: dint_hip.hip, stage_dictionary).
struct dict_view {
    const uint8_t* tables;      // heads (16 bytes per slot) | tails (32 bytes per slot) | goff (u32 per slot) | gtable (u32 payload words)
    const uint32_t* lds_image;  // [256 u16 zeros]{[hot meta of dictionary d]}[hot payloads as u16], hot_words long
    const dict_desc* descs;     // one per dictionary (multi: 6)
    uint32_t tables_bytes;
    uint32_t heads_base;        // byte offset of the heads inside `tables`: {metadata word, integers 0..5 as u16} per slot
    uint32_t tails_base;        // ... of the tails: integers 6..21 as u16 per slot
    uint32_t goff_base;         // ... of the slow path's offsets into gtable (u32 per slot)
    uint32_t gtable_base;       // ... of gtable
    uint32_t hot_words;         // multiple of 4
    dict_desc first;            // descs[0], for the single-dictionary kernel
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct decode_args {
    dict_view dict;
    const uint8_t* enc;
    uint64_t enc_bytes;
    const dint_unit* units;
    uint64_t n_units;
    uint32_t* out;
    uint64_t out_capacity;
    uint64_t* end_off;  // nullable
    uint32_t* queue;    // kQueueShards counters, kQueueStride words apart, zero at launch
    uint32_t n_shards;  // counters in use
    uint32_t only_full; // in-index path: decode units of exactly 256 integers only (tails are interpolative)
    const uint8_t* sched;  // nullable; per unit: c != 0 = a work item of the unit queue standing for c units (bundle_schedule_kernel)
    const uint32_t* items; // with sched: what the unit queue hands out, in order. Multi-dictionary kernel: the units on their
                           // own (sched == 1). Single-dictionary kernel: those and the bundles' first units —
    const uint8_t* item_cnt;  // ... with the units each item stands for (1: a unit on its own)
    const uint32_t* n_items;
    // with sched: the bundles, found chunk by chunk (64 consecutive units; a bundle does not cross chunks)
    const u32x4* urec;       // per unit: {in_off - chunk's in0, out_off - chunk's out0, packed (see bundle_schedule_kernel), 0}
    const uint64_t* cbase;   // per chunk: {in0, out0} = in_off / out_off of its first unit
    uint32_t* chunk_queue;   // a line of the launch's counters (zero at launch): word kClockWordAt: the clock; behind it kChunkShards lines: the chunks' ticket counters
    const uint32_t* spans; // nullable; per unit an upper bound of its stream bytes (else: up to the next unit's start)
    uint32_t plus_one;     // in-index freqs parts: every decoded integer + 1 (dict_posting_list.hpp:164-169)
    // in-index docs parts (units = 256-posting blocks): the gaps leave the kernel as docIDs — docid_i = base +
    // sum_{j<=i} (gap_j + 1) - 1 (dict_posting_list.hpp:111-124, :304), one wave scan per block in the expansion.
    const uint32_t* unit_base;  // nullable; per unit: the block's docID base
    uint8_t* gaps_left;         // with unit_base; per unit, zero at launch: set where a block had to be left as gaps (it
                                // held a slow codeword) for the flagged fix-up
    uint32_t chunk_split_log2;  // the bundle path's tickets: a chunk in 2^this parts (0..4); anything else: by the launch's size
    uint64_t* clock;            // where the launch's first wave leaves its cycle count: a word of the DICTIONARY's own counter lines
                                // (dint_last_kernel_clock_mhz reads it: never a word of a block table's counters, which a table's
                                // destruction would take away under the reader)
};

struct __attribute__((packed, aligned(1))) u32x4_a1 {
    u32x4 v;
};
struct __attribute__((packed, aligned(1))) u32x2_a1 {
    u32x2 v;
};
struct __attribute__((packed, aligned(1))) u32_a1 {
    uint32_t v;
};
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) uint32_t lds_u32;

__device__ __forceinline__ uint32_t lane_id() {
    return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}

// Inclusive prefix sum over the 64 lanes, in registers: four row_shr steps inside each row of 16, then
// row_bcast:15 / row_bcast:31 across rows (gfx9 DPP) — written out: the builtin form compiled to three
// instructions a step (mov 0, mov_dpp, add) wherever the combine pass gave up. A VALU result needs two wait
// states before a DPP instruction reads it.
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t x) {
    asm("s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_add_u32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(x));
    return x;
}

// Inclusive prefix maximum over the 64 lanes (same DPP pattern; zero fill is neutral for unsigned max).
__device__ __forceinline__ uint32_t wave_inclusive_max(uint32_t x) {
    auto mx = [](uint32_t a, uint32_t b) { return a > b ? a : b; };
    x = mx(x, uint32_t(__builtin_amdgcn_update_dpp(0u, x, 0x111, 0xf, 0xf, false)));
    x = mx(x, uint32_t(__builtin_amdgcn_update_dpp(0u, x, 0x112, 0xf, 0xf, false)));
    x = mx(x, uint32_t(__builtin_amdgcn_update_dpp(0u, x, 0x114, 0xf, 0xf, false)));
    x = mx(x, uint32_t(__builtin_amdgcn_update_dpp(0u, x, 0x118, 0xf, 0xf, false)));
    x = mx(x, uint32_t(__builtin_amdgcn_update_dpp(x, x, 0x142, 0xa, 0xf, false)));
    x = mx(x, uint32_t(__builtin_amdgcn_update_dpp(x, x, 0x143, 0xc, 0xf, false)));
    return x;
}

// The value of the lane below (lane 0: zero) / above (lane 63: zero): one DPP move instead of a trip
// through the LDS crossbar (ds_bpermute, what __shfl_up / __shfl_down compile to).
__device__ __forceinline__ uint32_t from_lane_below(uint32_t x) {
    return __builtin_amdgcn_update_dpp(0u, x, 0x138, 0xf, 0xf, true);  // wave_shr:1
}
__device__ __forceinline__ uint32_t from_lane_above(uint32_t x) {
    return __builtin_amdgcn_update_dpp(0u, x, 0x130, 0xf, 0xf, true);  // wave_shl:1
}

__device__ __forceinline__ uint32_t readlane(uint32_t x, uint32_t l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ uint32_t uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ uint64_t uniform64(uint64_t x) {
    return (uint64_t(uniform(uint32_t(x >> 32))) << 32) | uniform(uint32_t(x));
}

// Orders this wave's LDS traffic between phases that communicate across lanes.
// LDS operations of one wave execute in issue order, so no hardware barrier is
// needed; this only stops the compiler from moving accesses across the point.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// How load_lane_slots addresses the stream: a generic pointer (flat loads), or one in the global address space.
template <bool GLOBAL>
struct slot_stream_ptr {
    typedef const uint8_t* type;
    typedef const u32x2_a1* x2;
    typedef const u32_a1* x1;
};
template <>
struct slot_stream_ptr<true> {
    typedef const __attribute__((address_space(1))) uint8_t* type;
    typedef const __attribute__((address_space(1))) u32x2_a1* x2;
    typedef const __attribute__((address_space(1))) u32_a1* x1;
};

// kSPL consecutive slots of one lane (16-bit slots: 8 bytes; `narrow`, 8-bit slots: 4 bytes) from an
// arbitrary byte address (SURVEY H4). `tile_byte` is the (wave-uniform) offset of the tile's
// first slot: when the whole tile lies inside the buffer — every tile but the stream's last —
// this is one plain load whose result nothing touches until the tile is unpacked, two tiles
// later. Otherwise it never reads past the buffer: the tail lanes load the final bytes and
// shift (bytes past the end read as zero), which waits for the data on the spot.
// (`narrow` is a compile-time constant in the single-dictionary kernel and wave-uniform in the multi one.)
// GLOBAL: the load is a global_load, not a flat_load (`enc` reaches the kernel inside a struct, so the compiler takes it for
// a generic pointer): a flat load in flight counts on the LDS counter as well as on vector memory's, and the compiler waits
// for it on both.
// INSIDE: the caller has checked that the whole tile lies inside the buffer.
template <bool GLOBAL = false, bool INSIDE = false>
__device__ __forceinline__ uint64_t load_lane_slots(bool narrow, const uint8_t* enc_generic, uint64_t tile_byte, uint32_t lane,
                                                    uint64_t enc_bytes) {
    typedef typename slot_stream_ptr<GLOBAL>::type byte_ptr;
    typedef typename slot_stream_ptr<GLOBAL>::x2 x2_ptr;
    typedef typename slot_stream_ptr<GLOBAL>::x1 x1_ptr;
    const byte_ptr enc = (byte_ptr)enc_generic;
    const uint32_t kBytes = narrow ? 4u : 8u;
    const uint64_t byte_off = tile_byte + uint64_t(kBytes) * lane;
    if (INSIDE || (tile_byte <= enc_bytes && enc_bytes - tile_byte >= uint64_t(kBytes) * kWave)) {  // wave-uniform
        if (GLOBAL && !narrow) {  // (the wave-uniform part of the address first, then the lane's 32-bit offset)
            const u32x2 r = ((x2_ptr)((enc + tile_byte) + kBytes * lane))->v;
            return (uint64_t(r.y) << 32) | r.x;
        }
        if (!narrow) {
            const u32x2 r = ((x2_ptr)(enc + byte_off))->v;
            return (uint64_t(r.y) << 32) | r.x;
        }
        return ((x1_ptr)(enc + byte_off))->v;
    }
    const uint64_t last_valid = enc_bytes - kBytes;  // enc_bytes >= 8 is checked by the host
    const uint64_t o = byte_off < last_valid ? byte_off : last_valid;
    const uint64_t over = byte_off - o;  // 0 for all but the tail lanes
    uint64_t q;
    if (!narrow) {
        const u32x2 r = ((x2_ptr)(enc + o))->v;
        q = (uint64_t(r.y) << 32) | r.x;
    } else {
        q = ((x1_ptr)(enc + o))->v;
    }
    return over < kBytes ? q >> (8 * uint32_t(over)) : 0ull;
}

struct tile_regs {
    uint32_t s[kSPL];  // slot values
    uint32_t m[kSPL];  // metadata of each slot read as a codeword (garbage for payload slots)
};
struct meta_regs {     // the metadata of a tile's hot slots on its way in (LDS); the cold slots' comes with their heads
    uint32_t h[kSPL];
};
struct head_regs {     // per cold slot: the 16-byte head of its dictionary entry — metadata word + its first 6 integers
    u32x4 q[kSPL];     // (later in the tile: the next 8 integers of the entries that have them)
};

__device__ __forceinline__ void unpack_slots(bool narrow, uint64_t raw, tile_regs& t) {
    if (!narrow) {
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) t.s[k] = uint32_t(raw >> (16 * k)) & 0xFFFFu;
    } else {
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) t.s[k] = uint32_t(raw >> (8 * k)) & 0xFFu;
    }
}

// Slot classification table. Whether a slot is a codeword header or an exception
// payload depends on its predecessors; per lane (4 consecutive slots) the outcome is a
// function of how many payload slots the previous lane still owes (st_in) and of the
// digits d_k = 2 - min(slot_k, 2) (0: ordinary, 1: value 1, 2: value 0). One u16 row per
// (st_in, d3 d2 d1 d0 in base 3):
//   bits 0-3 payload slots | 4-7 exception headers | 8-10 st_out |
//   bit 11, bits 12-13, bits 14-15: headers before slot 1, 2, 3 (ordinal inside the lane)
// Rows [0, 243) are for 16-bit slots (payloads of 1 / 2 slots), rows [243, 648) for
// 8-bit slots (2 / 4 slots).
constexpr uint32_t kRows16 = 3 * 81, kRows8 = 5 * 81;
constexpr uint32_t kClassRows = kRows16 + kRows8;

__device__ __forceinline__ uint32_t class_row(bool w16, uint32_t st, uint32_t digits) {
    uint32_t pay = 0, exc = 0, hdr_before = 0, ords = 0;
    for (uint32_t k = 0; k != 4; ++k) {
        const uint32_t d = digits % 3;
        digits /= 3;
        if (k == 1) ords |= hdr_before << 11;
        if (k == 2) ords |= hdr_before << 12;
        if (k == 3) ords |= hdr_before << 14;
        const bool p = st != 0;
        const bool e = !p && d != 0;
        pay |= uint32_t(p) << k;
        exc |= uint32_t(e) << k;
        hdr_before += p ? 0u : 1u;
        st = p ? st - 1 : (e ? (w16 ? (d == 1 ? 2u : 1u) : (d == 1 ? 4u : 2u)) : 0u);
    }
    return pay | (exc << 4) | (st << 8) | ords;
}

__device__ __forceinline__ void build_class_table(uint16_t* table) {
    for (uint32_t i = threadIdx.x; i < kClassRows; i += kBlockThreads) {
        const bool w16 = i < kRows16;
        const uint32_t j = w16 ? i : i - kRows16;
        table[i] = uint16_t(class_row(w16, j / 81, j % 81));
    }
}

// Section marks for tools/isa_count.py (comments in the assembly under -DDINT_MARKS; nothing otherwise).
#ifdef DINT_MARKS
#define MARK(name) asm volatile("; MARK " name)
#else
#define MARK(name) do {} while (0)
#endif
// Under -DDINT_PROFILE (a diagnostic build, tools/variants/) the marks also stamp the shader clock.
#ifdef DINT_PROFILE
#include "dint_profile.hpp"
#else
struct prof_t {};
#define SECTION(pf, id, name) MARK(name)
#define QTRACE(k) do { } while (0)
#endif

