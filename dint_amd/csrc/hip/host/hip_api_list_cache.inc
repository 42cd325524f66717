// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": a posting list decoded once, its blocks then served from host memory (dint_list_cache_*).
// ---- a posting list decoded once, its blocks then served from host memory ---------------------------------------
struct dint_list_cache {
    size_t n_blocks = 0, list_bytes = 0;
    bool with_freqs = false;
    std::vector<dint_block_ref> blocks;   // in_off: the docs part's offset inside the list
    std::vector<uint64_t> docs_end, freqs_end;
    std::vector<uint32_t> gaps, freqs;    // what Coder::decode returns for the docs / freqs parts, blocks back to back
};

int dint_list_cache_create(const dint_dict* docs_c, const dint_dict* freqs_dict, const uint8_t* list, size_t list_bytes,
                           dint_list_cache** out) {
    if (!docs_c || !list || !out || list_bytes < 2) return DINT_ERR_ARG;
    *out = nullptr;
    if (freqs_dict && (freqs_dict->device != docs_c->device || freqs_dict->kind != docs_c->kind)) return DINT_ERR_ARG;
    dint_block_ref* blocks = nullptr;
    size_t n_blocks = 0;
    uint64_t total = 0;
    const uint64_t zero = 0;
    int st = dint_index_posting_lists(list, list_bytes, &zero, 1, &blocks, &n_blocks, &total);
    if (st != DINT_OK) return st;
    auto* c = new (std::nothrow) dint_list_cache();
    if (!c) {
        dint_free(blocks);
        return DINT_ERR_NOMEM;
    }
    c->n_blocks = n_blocks;
    c->list_bytes = list_bytes;
    c->with_freqs = freqs_dict != nullptr;
    c->blocks.assign(blocks, blocks + n_blocks);
    dint_free(blocks);
    c->docs_end.assign(n_blocks, 0);
    c->freqs_end.assign(n_blocks, 0);
    c->gaps.assign(total, 0);
    if (freqs_dict) c->freqs.assign(total, 0);
    dint_dict* dd = const_cast<dint_dict*>(docs_c);
    dint_dict* fdd = const_cast<dint_dict*>(freqs_dict);
    // (the docs dictionary's workspace and both dictionaries' schedule memory: one call at a time on either)
    std::unique_lock<std::mutex> lock(dd->host_mutex, std::defer_lock), flock;
    if (fdd && fdd != dd) {
        flock = std::unique_lock<std::mutex>(fdd->host_mutex, std::defer_lock);
        std::lock(lock, flock);
    } else {
        lock.lock();
    }
    // device: [index, padded][blocks][units][funits][docs ends][freqs ends][spans][fspans][tails + count][docs out][freqs out]
    const size_t padded = list_bytes + 16;
    const size_t b_index = up256(padded), b_blocks = up256(n_blocks * sizeof(dint_block_ref)), b_units = up256(n_blocks * sizeof(dint_unit)),
                 b_u64 = up256(n_blocks * 8), b_u32 = up256((n_blocks + 1) * 4), b_out = up256(size_t(total) * 4);
    const size_t dev_bytes = b_index + b_blocks + 2 * b_units + 2 * b_u64 + 3 * b_u32 + 2 * b_out;
    const size_t pin_bytes = std::max(b_index + b_blocks, 2 * b_u64 + 2 * b_out);
    auto fail = [&](int code) {
        delete c;
        return code;
    };
    st = host_workspace(dd, pin_bytes, dev_bytes);
    if (st != DINT_OK) return fail(st);
    hipStream_t s = dd->host_stream;
    uint8_t* p = dd->d_host;
    uint8_t* const d_index = p;
    p += b_index;
    auto* d_blocks = reinterpret_cast<dint_block_ref*>(p);
    p += b_blocks;
    auto* d_units = reinterpret_cast<dint_unit*>(p);
    p += b_units;
    auto* d_funits = reinterpret_cast<dint_unit*>(p);
    p += b_units;
    auto* d_dends = reinterpret_cast<uint64_t*>(p);
    p += b_u64;
    auto* d_fends = reinterpret_cast<uint64_t*>(p);
    p += b_u64;
    auto* d_spans = reinterpret_cast<uint32_t*>(p);
    p += b_u32;
    auto* d_fspans = reinterpret_cast<uint32_t*>(p);
    p += b_u32;
    auto* d_tails = reinterpret_cast<uint32_t*>(p);
    p += b_u32;
    auto* d_gaps = reinterpret_cast<uint32_t*>(p);
    p += b_out;
    auto* d_freqs = reinterpret_cast<uint32_t*>(p);
    std::memcpy(dd->h_pin, list, list_bytes);
    std::memset(dd->h_pin + list_bytes, 0, b_index - list_bytes);
    std::memcpy(dd->h_pin + b_index, c->blocks.data(), n_blocks * sizeof(dint_block_ref));
    auto hip = [&](hipError_t e, const char* what) { return hip_ok(e, what) ? DINT_OK : DINT_ERR_HIP; };
    if ((st = hip(hipMemcpyAsync(dd->d_host, dd->h_pin, b_index + b_blocks, hipMemcpyHostToDevice, s), "hipMemcpyAsync(list)")) != DINT_OK) return fail(st);
    if ((st = hip(hipMemsetAsync(d_dends, 0, 2 * b_u64, s), "hipMemsetAsync")) != DINT_OK) return fail(st);
    if ((st = hip(hipMemsetAsync(d_tails + n_blocks, 0, 4, s), "hipMemsetAsync")) != DINT_OK) return fail(st);
    const uint32_t tb = 256, grid = uint32_t((n_blocks + tb - 1) / tb);
    const uint32_t tgrid = uint32_t((n_blocks + kTailLanes - 1) / kTailLanes);  // (sized for "every block is short": at most one is)
    hipLaunchKernelGGL(collect_tails_kernel, dim3(grid), dim3(tb), 0, s, d_blocks, uint64_t(n_blocks), d_tails, d_tails + n_blocks);
    hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, d_blocks, static_cast<const uint64_t*>(nullptr), uint64_t(n_blocks),
                       uint64_t(padded), d_units, d_spans, static_cast<uint32_t*>(nullptr));
    // docs parts as the Coder returns them (gaps), where they end; then the freqs parts from there
    dd->host_sched.valid = false;
    decode_request docs;
    docs.dict = docs_c, docs.enc = d_index, docs.enc_bytes = padded, docs.n_units = n_blocks, docs.out_capacity = total, docs.stream = s;
    docs.only_full = 1, docs.units = d_units, docs.spans = d_spans, docs.out = d_gaps, docs.end_off = d_dends, docs.cache = &dd->host_sched;
    st = launch_decode(docs);
    if (st != DINT_OK) return fail(st);
    hipLaunchKernelGGL(interpolative_tails_kernel, dim3(tgrid), dim3(64), kTailLdsBytes, s, d_index, uint64_t(padded), d_blocks,
                       static_cast<const uint64_t*>(nullptr), d_tails, d_tails + n_blocks, d_gaps, uint64_t(total), d_dends, 0u);
    if (freqs_dict) {
        hipLaunchKernelGGL(blocks_to_units_kernel, dim3(grid), dim3(tb), 0, s, d_blocks, d_dends, uint64_t(n_blocks), uint64_t(padded), d_funits,
                           d_fspans, static_cast<uint32_t*>(nullptr));
        fdd->host_sched.valid = false;  // (the freqs dictionary's own schedule memory)
        decode_request freqs = docs;
        freqs.dict = freqs_dict;
        freqs.units = d_funits, freqs.spans = d_fspans, freqs.out = d_freqs, freqs.end_off = d_fends, freqs.cache = &fdd->host_sched;
        st = launch_decode(freqs);
        if (st != DINT_OK) return fail(st);
        hipLaunchKernelGGL(interpolative_tails_kernel, dim3(tgrid), dim3(64), kTailLdsBytes, s, d_index, uint64_t(padded), d_blocks, d_dends, d_tails,
                           d_tails + n_blocks, d_freqs, uint64_t(total), d_fends, 0u);
    }
    if ((st = hip(hipGetLastError(), "launch")) != DINT_OK) return fail(st);
    uint8_t* hp = dd->h_pin;
    if ((st = hip(hipMemcpyAsync(hp, d_dends, 2 * b_u64, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(ends)")) != DINT_OK) return fail(st);
    if ((st = hip(hipMemcpyAsync(hp + 2 * b_u64, d_gaps, (freqs_dict ? 2 : 1) * b_out, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(out)")) != DINT_OK)
        return fail(st);
    if ((st = hip(hipStreamSynchronize(s), "hipStreamSynchronize")) != DINT_OK) return fail(st);
    std::memcpy(c->docs_end.data(), hp, n_blocks * 8);
    std::memcpy(c->freqs_end.data(), hp + b_u64, n_blocks * 8);
    std::memcpy(c->gaps.data(), hp + 2 * b_u64, size_t(total) * 4);
    if (freqs_dict) std::memcpy(c->freqs.data(), hp + 2 * b_u64 + b_out, size_t(total) * 4);
    *out = c;
    return DINT_OK;
}

void dint_list_cache_destroy(dint_list_cache* c) { delete c; }

namespace {
enum class cache_part { either, docs, freqs };

// The part of n integers that starts at in_offset. A docs part without bits (one posting, or consecutive docIDs: a sum of
// zero) has no bytes, and the freqs part of its block starts where it does: `either` (the offset alone) answers with the docs
// part there; a caller that knows which part it asks for — the Coder's sum_of_values says — gets that one.
int list_cache_serve(const dint_list_cache* c, size_t in_offset, cache_part part, uint32_t* out, size_t n, size_t* consumed) {
    if (!c || (!out && n)) return DINT_ERR_ARG;
    if (consumed) *consumed = 0;
    // the block whose docs part starts at in_offset, else the one whose freqs part does (where its docs part ended)
    auto it = std::lower_bound(c->blocks.begin(), c->blocks.end(), in_offset,
                               [](const dint_block_ref& b, size_t off) { return b.in_off < off; });
    size_t b = size_t(it - c->blocks.begin());
    const bool docs_here = b < c->n_blocks && c->blocks[b].in_off == in_offset;
    if (docs_here && part != cache_part::freqs) {
        if (n != c->blocks[b].n) return DINT_ERR_ARG;
        if (c->docs_end[b] < in_offset) return DINT_ERR_FORMAT;  // (a block the decode did not reach: its end was never written)
        std::memcpy(out, c->gaps.data() + c->blocks[b].out_off, n * 4);
        if (consumed) *consumed = size_t(c->docs_end[b] - in_offset);
        return DINT_OK;
    }
    if (!c->with_freqs || part == cache_part::docs) return DINT_ERR_ARG;
    if (!(docs_here && c->docs_end[b] == in_offset)) {  // (else: this block's own freqs part, behind a docs part of no bytes)
        if (b == 0) return DINT_ERR_ARG;
        b -= 1;  // the last block that starts before in_offset
    }
    if (c->docs_end[b] != in_offset || n != c->blocks[b].n) return DINT_ERR_ARG;
    if (c->freqs_end[b] < in_offset) return DINT_ERR_FORMAT;
    std::memcpy(out, c->freqs.data() + c->blocks[b].out_off, n * 4);
    if (consumed) *consumed = size_t(c->freqs_end[b] - in_offset);
    return DINT_OK;
}
}  // namespace

int dint_list_cache_decode(const dint_list_cache* c, size_t in_offset, uint32_t* out, size_t n, size_t* consumed) {
    return list_cache_serve(c, in_offset, cache_part::either, out, n, consumed);
}

int dint_list_cache_decode_part(const dint_list_cache* c, size_t in_offset, uint32_t sum_of_values, uint32_t* out, size_t n,
                                size_t* consumed) {
    return list_cache_serve(c, in_offset, sum_of_values == 0xFFFFFFFFu ? cache_part::freqs : cache_part::docs, out, n, consumed);
}

