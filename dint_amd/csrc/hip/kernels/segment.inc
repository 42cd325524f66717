// Part of dint_kernels.hpp (included from there, in order, inside namespace dint_dev): decode_segment: one unit's tiles, three in flight per wave.
// ROUNDS x GROUPS x 256 = outputs per expansion batch: 2 x 4 for the long single-dictionary
// segments; a multi-dictionary segment is one block of at most 256 integers, 1 x 1.
// W = 16 / 8: the slot width; 0: `narrow_rt` says (wave-uniform). CHAINED = 1 / 0, or -1: `chained_rt` says.
// (The multi-dictionary kernel has ONE instantiation for both widths, chained or not: with four, inlined side by
// side, the register allocator spilled 127 registers to scratch.)
// TOUCH: the vroom single-dictionary launches (decode_unit_single) — the prologue's trip to memory brings the rest of the unit's
// stream into L2 as well (dint_stream_touch.hpp). Every other segment compiles to the code it had without it.
template <int W, uint32_t ROUNDS, uint32_t GROUPS, int CHAINED_T, bool TOUCH = false>
__device__ __forceinline__ uint64_t decode_segment(const decode_args& a, const wave_ctx& c, const dict_desc& dd, uint64_t in_off,
                                                   uint32_t n, uint32_t* const out, chain_io& ch, prof_t& pf,
                                                   bool narrow_rt = false, bool chained_rt = false,
                                                   const uint32_t* block_base = nullptr, uint8_t* gaps_left = nullptr,
                                                   uint32_t touch_span = 0) {  // TOUCH: the unit's stream bytes (wave-uniform), 0: not known
    SECTION(pf, 11, "segment_prologue");
    docid_bases gb;  // (in-index docs part: the block's docID base, asked for now — see docid_bases)
    if (block_base != nullptr) gb.v = *block_base;
    const bool narrow = W == 0 ? narrow_rt : W == 8;
    const bool CHAINED = CHAINED_T < 0 ? chained_rt : CHAINED_T != 0;
    const uint32_t kSlotBytes = narrow ? 1u : 2u;
    const uint32_t kTileBytes = kTileSlots * kSlotBytes;
    const uint16_t* const rows = c.cls + (!narrow ? 0 : kRows16);
    const uint32_t lane = c.lane;
    const uint32_t hot_k = dd.hot_k;
    // hardware bounds: nothing past this segment's n integers can be written
    uint32_t* const out_u = reinterpret_cast<uint32_t*>(uniform64(reinterpret_cast<uint64_t>(out)));
    const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(out_u, 0, int(uniform(n) * 4), 0x00020000);
    uint8_t* const lds_rw = reinterpret_cast<uint8_t*>(const_cast<uint32_t*>(c.lds));
    const uint32_t stage_byte0 = uint32_t(reinterpret_cast<const uint8_t*>(stage_of(c.scratch)) - lds_rw);  // the cells, as LDS byte addresses

    // pipeline: tile t in `cur` (slots + metadata; the rows of its cold slots on their way into `rr`), tile
    // t+1's slots in `nxt` (its metadata requested half-way through tile t, its rows at the end of tile t),
    // tile t+2's slots in raw2, tile t+3's requested at the top of tile t.
    // kPaired (the single-dictionary segments, DINT_SLOT_BURST 2): the slots are requested two tiles at a time — tiles
    // t+2 and t+3 back to back at the top of every ODD tile t, nothing at the top of the even ones (the prologue has
    // asked for tiles 0, 1 and 2). The 128-byte line that two neighbouring tiles share is then asked for twice within
    // a few cycles, not a tile-time (about 10 k cycles of other traffic through the L2) apart: it comes from HBM once,
    // and HBM sees 1 KB per request point, half as many of them. An odd tile holds t+1 (nxt_raw) and the pair, an
    // even one t+1 and t+2 (raw2, and a raw3 nobody reads): six registers of slots at the most, as before.
    constexpr bool kPaired = DINT_SLOT_BURST == 2 && W == 16 && CHAINED_T == 0;
    // ... and their loads are global loads (load_lane_slots<true>), not flat ones: vector memory's counter alone.
    constexpr bool kGlobalSlots = DINT_SLOT_GLOBAL != 0 && W == 16 && CHAINED_T == 0;
    constexpr bool kLateSlots = DINT_SLOT_LATE != 0 && W == 16 && CHAINED_T == 0;  // DINT_SLOT_BURST 1 only: see the loop top
    constexpr bool kTouch = TOUCH && kPaired && DINT_STREAM_TOUCH_LANES != 0;
    const uint64_t in_off_u = uniform64(in_off);
    uint64_t slot_byte = in_off_u;  // first byte of the tile whose slots are loaded next (wave-uniform)
    // kPaired: the stream's bytes from the unit's first on, saturated to 32 bits (wave-uniform)
    uint32_t room = 0;
    if (kPaired && in_off_u <= a.enc_bytes) room = uniform(a.enc_bytes - in_off_u < 0xFFFFFFFFull ? uint32_t(a.enc_bytes - in_off_u) : 0xFFFFFFFFu);
    tile_regs cur;
    uint64_t nxt_raw;  // tile t+1's slots, packed as they were loaded: unpacked where they are used (two registers instead of four
                       // across the front end of tile t, where the register file is fullest)
    meta_regs mr;
    head_regs hr;  // (deliberately uninitialised: each register is written and read under the same lane predicate)
    uint64_t raw1, raw2 = 0;
    if (CHAINED) {  // tiles 0 and 1 arrived with the previous block (or were requested by the caller)
        unpack_slots(narrow, chain_tile(narrow, ch.data, 0, lane), cur);
        raw1 = chain_tile(narrow, ch.data, 1, lane);
        slot_byte += kTileBytes;  // the pipeline is one tile shorter: tile t+2's slots are requested in tile t
    } else {
        // (all three requested before the first is looked at: one trip to memory, not two)
        uint64_t raw0 = load_lane_slots<kGlobalSlots>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
        slot_byte += kTileBytes;
        raw1 = load_lane_slots<kGlobalSlots>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
        slot_byte += kTileBytes;
        raw2 = load_lane_slots<kGlobalSlots>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
        if (kTouch) {
            // ... and in the same trip the lines behind tile 2, a dword of each: lane l asks for the line at stream_touch's
            // first_line + 128 l and uses its value for nothing. The unit's pair requests — eight or nine more points at which
            // this wave would stand at the head of the CU's in-order return queue for an HBM latency — then find their lines in
            // L2. A plain load, consumed at the barrier the three tiles are consumed at: no wait and no request point of its own,
            // and its register is dead from there on. The lanes past the window ask for the window's last line again (a
            // clamp, not a branch of the lanes: one request more on a line already asked for); stream_touch keeps every line it
            // returns inside the stream, and a unit with no window skips the load (wave-uniform).
            // (The address is a wave-uniform base and the lane's 32-bit offset, like load_lane_slots' global form. Through a
            // buffer descriptor whose range clips the lanes, the descriptor's four scalars were spilled: 56 -> 67 spilled scalar
            // registers, which take a second vector register to hold, and decode_single_kernel spilled a vector register.)
            typedef slot_stream_ptr<true>::type stream_ptr;
            typedef slot_stream_ptr<true>::x1 dword_ptr;  // (a line of the STREAM: the buffer's own alignment is the caller's)
            // The window is the unit's own lines where decode_unit_single found its span in the table (unit_touch: up to
            // DINT_STREAM_TOUCH_LINES = 128 of them, through DINT_STREAM_TOUCH_PAST bytes behind the unit's end: the next unit's
            // first three tiles), the rule of n where it did not. A wave has 64 lanes: the lines from kOneLoad on are a SECOND
            // load in the same trip, lane l asking for line kOneLoad + l, clamped like the first — issued for the units that
            // have such lines (wave-uniform; nearly half of the bench's long units), consumed at the same barrier, dead behind it.
            constexpr uint32_t kOneLoad = DINT_STREAM_TOUCH_LANES;
            constexpr uint32_t kMaxLines = DINT_STREAM_TOUCH_LINES < 2 * kOneLoad ? DINT_STREAM_TOUCH_LINES : 2 * kOneLoad;
            const stream_touch_lines tw = unit_touch(in_off_u, uniform(n), uniform(touch_span), a.enc_bytes, kMaxLines);
            const uint32_t last = tw.lines - 1;
            uint32_t touched = 0, touched2 = 0;
            if (tw.lines != 0) {
                const uint32_t last0 = last < kOneLoad - 1 ? last : kOneLoad - 1;
                const uint32_t l = lane < last0 ? lane : last0;
                touched = ((dword_ptr)(((stream_ptr)a.enc + tw.first_line) + kTouchLineBytes * l))->v;
            }
            if (kMaxLines > kOneLoad && tw.lines > kOneLoad) {
                const uint32_t l = kOneLoad + lane < last ? kOneLoad + lane : last;
                touched2 = ((dword_ptr)(((stream_ptr)a.enc + tw.first_line) + kTouchLineBytes * l))->v;
            }
            asm volatile("" : "+v"(raw0), "+v"(raw1), "+v"(raw2), "+v"(touched), "+v"(touched2));
        } else {
            asm volatile("" : "+v"(raw0), "+v"(raw1), "+v"(raw2));
        }
        unpack_slots(narrow, raw0, cur);
    }
    ch.valid = false;
    // ---- classification of a tile's slots — which are an exception's payload, which exception headers — by table
    // lookup, repeated until the lane-to-lane carries agree. It needs the slots and the carry of the tile before and
    // nothing else, so it runs a tile AHEAD, before the tile's heads are requested: payload slots ask for none.
    struct tile_class {
        uint32_t row;        // the lane's classification row (kPlainRow: four codeword headers)
        uint32_t carry_out;  // payload slots the tile's last exception still owns in the next tile (wave-uniform)
        bool special;        // some slot is an exception header or payload (wave-uniform)
        bool tile_exc;       // some slot is an exception header (wave-uniform)
    };
    auto classify = [&](const tile_regs& tr, uint32_t carry_in) -> tile_class {
        tile_class k{kPlainRow, 0u, false, false};
        uint32_t smin = tr.s[0];
#pragma unroll
        for (uint32_t j = 1; j != kSPL; ++j) smin = smin < tr.s[j] ? smin : tr.s[j];
        k.special = __builtin_expect(__ballot(smin < 2) != 0 || carry_in != 0, 0);
        if (k.special) {
            // base-3 digits of the four slots: 2 - min(slot, 2)
            uint32_t lo = 0;
#pragma unroll
            for (uint32_t j = kSPL; j-- != 0;) lo = 3 * lo + (2u - (tr.s[j] < 2 ? tr.s[j] : 2u));
            uint32_t st_in = lane == 0 ? carry_in : 0u;
            uint32_t row;
            for (;;) {
                row = rows[st_in * 81 + lo];
                uint32_t prev = from_lane_below((row >> 8) & 7u);
                if (lane == 0) prev = carry_in;
                if (__ballot(prev != st_in) == 0) break;
                st_in = prev;
            }
            k.row = row;
            k.carry_out = readlane((row >> 8) & 7u, 63);
            k.tile_exc = __ballot((row & 0xF0u) != 0) != 0;
        }
        return k;
    };
    tile_class kc = classify(cur, 0u);
    request_metas(c, dd.hot_base, hot_k, dd.meta_base, cur, mr, hr, kc.row & 15u);
    // Everything loaded so far has landed before the loop is entered: inside it, a wait may only
    // ever sit before a tile's stores (see the notes below), never right after them.
    asm volatile("" : "+v"(raw1), "+v"(raw2));
    nxt_raw = raw1;

    uint32_t produced = 0;
    uint64_t tile_base = in_off_u; // byte offset of slot 0 of the current tile (wave-uniform)
    uint32_t end_slot = 0;
    MARK("loop_top");

    while (produced < n) {
        // The far prefetch — the slots of the tile after next, straight from HBM — goes out first: it has to
        // be back before this tile's expansion (every wait is a wait for everything), so it gets the whole
        // front end. (Requested at the wait point instead, as the youngest load in flight there, it would have
        // a whole tile; measured: no gain — the kernel waits for the vector-memory front end, not for HBM.)
        // (Not so where the loop is kPaired, see below: in the assembly THIS request sits in front of the s_waitcnt
        // vmcnt(0) that take_metas' barriers make the compiler write, and is waited for there, a few cycles after it went out.)
        uint64_t raw3;
        if (!kPaired && !kLateSlots) {
            slot_byte += kTileBytes;
            raw3 = load_lane_slots<kGlobalSlots>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
        }

        SECTION(pf, 1, "1_classify");
        // this tile's metadata: requested before the previous tile's stores (so this is no wait for them)
        take_metas(hot_k, mr, hr, cur);
        // kPaired: the pair t+2, t+3 at the top of the odd tiles — BEHIND the wait for this tile's metadata. With stores
        // in flight the compiler's wait is a wait for everything (loads and stores share one counter, and it counts
        // nothing once both kinds are pending): a load requested before it is waited for on the spot, at HBM latency.
        // Requested behind it, the pair has the tile's front end, up to the wait point, to land (the one-tile request moved
        // here on its own, DINT_SLOT_LATE: -2.9 to -4.0 % at 10^9 postings; the pairs: -6.7 to -7.1 %). Where the pair's 1 KB
        // does not lie inside the buffer, each load takes load_lane_slots' end-of-buffer path on its own, so the second of
        // a pair never reads past the stream either.
        // (t+2's slots go straight into raw2, which an odd tile finds dead — handed on to nxt_raw a tile ago —, t+3's into
        // raw3: the rotation at the tile's end is the same for both parities, and an even tile hands on a raw3 nobody reads.
        // The parity needs no state: an odd tile finds the last request one tile ahead of it, an even one two.)
        if (!kPaired && kLateSlots) {  // (the A/B build that moves the one-tile request behind the wait and changes nothing else)
            slot_byte += kTileBytes;
            raw3 = load_lane_slots<kGlobalSlots>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
        }
        if (kPaired) {
            if (uint32_t(slot_byte - tile_base) == kTileBytes) {
                const uint64_t pair_byte = slot_byte + kTileBytes;
                slot_byte += 2 * kTileBytes;
                // (one 32-bit test for the pair, everywhere but at the stream's end: offsets inside a unit fit 32 bits)
                if (uint32_t(slot_byte - in_off_u) + kTileBytes <= room) {
                    raw2 = load_lane_slots<kGlobalSlots, true>(narrow, a.enc, pair_byte, lane, a.enc_bytes);
                    raw3 = load_lane_slots<kGlobalSlots, true>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
                } else {
                    raw2 = load_lane_slots<kGlobalSlots>(narrow, a.enc, pair_byte, lane, a.enc_bytes);
                    raw3 = load_lane_slots<kGlobalSlots>(narrow, a.enc, slot_byte, lane, a.enc_bytes);
                }
            } else {
                asm volatile("" : "=v"(raw3));  // (no instruction: the even tiles' raw3 is whatever the registers hold)
            }
        }
        // ---- 1. classification: done a tile ago (kc) ----
        const bool special = kc.special;
        const uint32_t row = kc.row;
        const uint32_t carry_out = kc.carry_out;
        const bool tile_exc = kc.tile_exc;

        SECTION(pf, 2, "2_sizes");
        // ---- 2. sizes, offsets; where each codeword's integers are -----------------------------------
        tile_slots t;
        // A payload slot decodes to nothing and takes nothing: its metadata word (whatever its value looks up) becomes
        // zero, and the 1 of "size - 1" is its live bit. An exception header needs no special case here: the
        // metadata of the two markers says one integer from one staging cell (stage_dictionary, choose_hot_set).
        uint32_t lv1[kSPL] = {1u, 1u, 1u, 1u};
        if (special) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) {
                cur.m[k] &= uint32_t(__builtin_amdgcn_sbfe(~row, k, 1));
                lv1[k] = __builtin_amdgcn_ubfe(~row, k, 1);
            }
        }
        // (behind the mask: a payload slot asked for no head, what its register holds is stale)
        const bool tile_slow_dict = __ballot(((cur.m[0] | cur.m[1] | cur.m[2] | cur.m[3]) & kMetaSlow) != 0) != 0;
        uint32_t e[kSPL];  // size - 1
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) {
            e[k] = cur.m[k] >> 24;
            t.need[k] = __builtin_amdgcn_ubfe(cur.m[k], 20, 2);
            t.src2[k] = cur.m[k] & kMetaOffMask;  // hot: the image (runs: the zeros); cold, slow: zero for now
        }
        // An exception's literal rides into its staging cell the way a cold codeword's first integers do: in the second
        // word of the slot's head register (the integers of a cell start 4 bytes in), 32 bits wide. The expansion gathers
        // its low half like any other integer, and — told by bit 0 of the source address — the upper half of one >= 65536.
        bool wide[kSPL] = {false, false, false, false};
        if (tile_exc) {
            // the 32 bits of the stream behind each slot: the lane's later slots, then the next lane's first ones (lane
            // 63: the next tile's; what lane 0 of the next tile holds is read with every lane enabled: a cross-lane read
            // of a value computed under `lane == 63` would find lane 0's register untouched)
            uint32_t w32[kSPL];
            if (!narrow) {
                const uint32_t p01 = (cur.s[1] << 16) | cur.s[0], p23 = (cur.s[3] << 16) | cur.s[2];
                const uint32_t next0 = readlane(uint32_t(nxt_raw), 0);  // (the next tile's first two slots, as packed)
                uint32_t nlo = from_lane_above(p01);
                if (lane == 63) nlo = next0;
                w32[0] = __builtin_amdgcn_alignbit(p23, p01, 16);
                w32[1] = p23;
                w32[2] = __builtin_amdgcn_alignbit(nlo, p23, 16);
                w32[3] = nlo;
            } else {
                const uint32_t b = cur.s[0] | (cur.s[1] << 8) | (cur.s[2] << 16) | (cur.s[3] << 24);
                const uint32_t next0 = readlane(uint32_t(nxt_raw), 0);  // (the next tile's first four 8-bit slots, as packed)
                uint32_t nlo = from_lane_above(b);
                if (lane == 63) nlo = next0;
                w32[0] = __builtin_amdgcn_alignbit(nlo, b, 8);
                w32[1] = __builtin_amdgcn_alignbit(nlo, b, 16);
                w32[2] = __builtin_amdgcn_alignbit(nlo, b, 24);
                w32[3] = nlo;
            }
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) {
                const uint32_t excM = uint32_t(__builtin_amdgcn_sbfe(row, 4 + k, 1));
                // marker 0: the 16 bits behind it; marker 1: all 32 (0 - marker = which)
                const uint32_t lit = w32[k] & ((0u - cur.s[k]) | 0xFFFFu) & excM;
                hr.q[k].y = (hr.q[k].y & ~excM) | lit;
                wide[k] = lit > 0xFFFFu;
            }
        }
        t.off[0] = 0;
        t.off[1] = e[0] + lv1[0];
        t.off[2] = t.off[1] + e[1] + lv1[1];
        t.off[3] = t.off[2] + e[2] + lv1[2];
        t.lsum = t.off[3] + e[3] + lv1[3];
        uint32_t hdrcnt = 4;
        uint32_t pincl;
        if (special) {
            hdrcnt = uint32_t(__builtin_popcount(~row & 15u));
            pincl = wave_inclusive_sum((hdrcnt << 24) | t.lsum);
        } else {
            pincl = wave_inclusive_sum(t.lsum);  // (the ordinals of a plain tile are 4 lane + k)
        }
        t.obase = (pincl & 0xFFFFFFu) - t.lsum;    // first output of this lane's codewords
        const uint32_t remaining = n - produced;
        t.total = readlane(pincl, 63) & 0xFFFFFFu;
        const bool last_tile = t.total >= remaining;
        const bool plain = !special && !last_tile && t.total <= ROUNDS * GROUPS * 256;
        uint32_t slowb = 0;  // bit k: slot k goes through slow_stores
        if (!plain) {
            t.row = row;
            t.liveb = ~row & 15u;
            // ordinal of this lane's first codeword (exclusive before the shift: the inclusive count can be 256)
            t.rbase = special ? (pincl - ((hdrcnt << 24) | t.lsum)) >> 24 : 4 * lane;
            t.nlive = hdrcnt;
            if (last_tile) {  // last tile of the segment: clamp, and find where the stream ends
                t.total = remaining;
                uint32_t cand = 0, lb = 0;
                t.nlive = 0;
#pragma unroll
                for (uint32_t k = 0; k != kSPL; ++k) {
                    const uint32_t pos = t.obase + t.off[k];
                    const bool act = ((t.liveb >> k) & 1u) != 0 && pos < remaining;
                    if (act) {
                        const bool exc = ((row >> (4 + k)) & 1u) != 0;
                        cand = kSPL * lane + k + 1 + (exc ? (!narrow ? cur.s[k] + 1 : 2 * cur.s[k] + 2) : 0u);
                        ++t.nlive;
                        lb |= 1u << k;
                    } else {
                        t.need[k] = 0;
                    }
                }
                t.liveb = lb;
                t.lsum = t.obase < remaining ? (t.obase + t.lsum < remaining ? t.lsum : remaining - t.obase) : 0u;
                const uint64_t am = __ballot(cand != 0);
                end_slot = readlane(cand, 63u - uint32_t(__builtin_clzll(am | 1ull)));
            }
            if (tile_slow_dict) {
#pragma unroll
                for (uint32_t k = 0; k != kSPL; ++k)
                    slowb |= ((cur.m[k] >> 22) & (t.liveb >> k) & ~(row >> (4 + k)) & 1u) << k;
            }
        } else if (tile_slow_dict) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) slowb |= ((cur.m[k] >> 22) & 1u) << k;
        }
        // ---- staging cells: exception literals and cold codewords --------------------------------------
        uint32_t cell_addr[kSPL];
        const uint32_t cells = allocate_cells(t, stage_byte0, cell_addr);
        if (cells > kStageCells) {  // wave-uniform; what lies past the staging area turns slow: zeros, then slow_stores
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k)
                if (t.need[k] != 0 && cell_addr[k] + 16 * t.need[k] > stage_byte0 + 16 * kStageCells) {
                    t.need[k] = 0;
                    slowb |= 1u << k;
                }
        }
#pragma unroll
        for (uint32_t k = 0; k != kSPL; ++k) t.src2[k] = t.need[k] != 0 ? cell_addr[k] : t.src2[k];
        const bool tile_wide = tile_exc && __ballot(wide[0] || wide[1] || wide[2] || wide[3]) != 0;
        const bool tile_slow = __ballot(slowb != 0) != 0;
        if (CHAINED && last_tile) {  // a chained segment asks for the next block as soon as it knows where this one ends
            const uint64_t nb = tile_base + uint64_t(kSlotBytes) * end_slot;
            if (ch.more && nb + 1 + kChainBytes <= a.enc_bytes) chain_request(a.enc, nb, lane, ch);
        }
        // ---- the wait point of the tile: everything prefetched has landed — nothing has been stored yet,
        // so this is no wait for store acknowledgements ("+v": from here on the values are the asm's, not a
        // load's — nothing for the compiler to wait for later, behind the stores)
        SECTION(pf, 8, "8_wait");
        uint64_t raw3w = raw3;
        asm volatile("" : "+v"(raw3w));
        if (kPaired) asm volatile("" : "+v"(raw2));  // (an odd tile: the pair's first half)
        if (CHAINED) asm volatile("" : "+v"(ch.sel), "+v"(ch.data.x), "+v"(ch.data.y), "+v"(ch.data.z), "+v"(ch.data.w));
        // the heads of this tile's cold codewords into their cells (the integers start 4 bytes in); the tails
        // of the large ones requested: integers 6..13 into the same registers, 14 and 15 into one more each
        uint32_t t3[kSPL];
        heads_into_cells<W == 16>(lds_rw, t, hr, wide);  // (W == 16: a single-dictionary kernel's segment)
        const bool tile_big = __ballot((t.need[0] | t.need[1] | t.need[2] | t.need[3]) > 1u) != 0;  // some codeword needs its tail
        if (tile_big) {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) {
                const uint32_t tail = c.tails_base + 32 * (dd.meta_base + cur.s[k]);
                if (t.need[k] > 1u) hr.q[k] = __builtin_amdgcn_raw_buffer_load_b128(c.rs_dict, tail, 0, 0);
                if (t.need[k] > 2u) t3[k] = __builtin_amdgcn_raw_buffer_load_b32(c.rs_dict, tail + 16, 0, 0);
            }
        }
        // (in-index docs part: the segment is one 256-posting block = one group of one tile; with a slow codeword in
        // it, or spread over two tiles — more than 256 slots: a block full of exceptions — it stays gaps and
        // the flagged fix-up (finalize_flagged_kernel, interpolative_tails_kernel) is told)
        const bool as_docids = block_base != nullptr && !tile_slow && produced == 0 && last_tile && t.total <= ROUNDS * GROUPS * 256;
        if (block_base != nullptr && !as_docids && lane == 0) *gaps_left = 1;
        gb.on = as_docids;
        if (block_base != nullptr) asm volatile("" : "+v"(gb.v));  // landed (behind this tile's wait point)
        expand_tile<ROUNDS, GROUPS>(t, plain, tile_wide, a.plus_one, gb, produced, c.lds, c.scratch, rs_out, lane, pf, [&]() {
#pragma unroll
            for (uint32_t k = 0; k != kSPL; ++k) asm volatile("" : "+v"(hr.q[k]), "+v"(t3[k]));
            if (tile_big) {
#pragma unroll
                for (uint32_t k = 0; k != kSPL; ++k) {
                    if (t.need[k] > 1u) *reinterpret_cast<u32x4*>(lds_rw + t.src2[k] + 12) = hr.q[k];
                    if (t.need[k] > 2u) *reinterpret_cast<uint32_t*>(lds_rw + t.src2[k] + 28) = t3[k];
                }
            }
            wave_lds_fence();
            // ---- the next tile's metadata (its slots are already here): the hot codewords' from LDS, the cold
            // ones' heads from L2 — requested before this tile's stores, so that the wait for them at the top of
            // the next tile is no wait for the stores (vmcnt is one in-order counter for loads AND stores on
            // gfx950). The last tile of a segment has no successor.
            SECTION(pf, 3, "3_prefetch");
            if (!last_tile) {
                // (the barrier: the compiler would unpack the slots and form the four head addresses a tile early — at the rotation,
                // where the value is first known — and spill them across this tile's front end: measured, 5 spilled registers
                // stored at every tile's end and reloaded here)
                asm volatile("" : "+v"(nxt_raw));
                tile_regs nxt;
                unpack_slots(narrow, nxt_raw, nxt);
                kc = classify(nxt, carry_out);
                request_metas(c, dd.hot_base, hot_k, dd.meta_base, nxt, mr, hr, kc.row & 15u);
            }
        });

        SECTION(pf, 10, "10_tail");
        if (tile_slow)
            slow_stores(narrow, c, t, slowb, a.plus_one, produced, n, a.enc + tile_base + uint64_t(kSPL * kSlotBytes) * lane, dd.hot_base,
                           hot_k, dd.meta_base, rs_out);
        SECTION(pf, 5, "10_rotate");
        produced += t.total;
        if (produced < n) tile_base += kTileBytes;

        // ---- rotate the pipeline ---------------------------------------------------
        asm volatile("" : "+v"(nxt_raw));  // (unpacked again here, not kept from the prefetch across the stores)
        unpack_slots(narrow, nxt_raw, cur);
        nxt_raw = CHAINED ? raw3w : raw2;
        raw2 = raw3w;
    }
    SECTION(pf, 13, "epilogue");
    return tile_base + uint64_t(kSlotBytes) * end_slot;
}

