// Part of dint_hip.hip (one translation unit; included from there, in order): extern "C": an index checked against its collection
// on the device (the reference's verify_collection, include/ds2i/verify_collection.hpp:7-52: DESIGN.md 4d-check).
// ---- index against collection -------------------------------------------------------------------
// The passes are dint_index_max_weights': consecutive blocks through gather_decode_pages into probe / fprobe. Beside
// them the expected side: per pass the host gathers the collection's postings of the pass's blocks — one memcpy per list
// segment, the view's lists being contiguous — into one of TWO pinned buffers, behind a check_page record per block, and
// a copy stream of the call's own brings it to the device while the pass before it decodes and compares on `stream`.
// Two events per buffer order the reuse: `copied` (the host may refill the pinned buffer, the compare may read the device
// copy) and `compared` (the copy stream may overwrite the device copy). Count and first-mismatch key come back in one
// small copy after the last pass; `got` comes from decoding that ONE block again (no thread of the compare writes it: a
// loser of the minimum could write after the winner).

// A pass holds at most this many pages whatever DINT_OPT_QUERY_OR_PASS_PAGES allows: 2^14 pages are 4 Mi postings, 32.25 MiB
// of records, docIDs and freqs per staging buffer. The results do not depend on it (sums and minima).
constexpr size_t kCheckPassPages = size_t(1) << 14;
// The staging buffers in use, of the handle's two. -DDINT_CHECK_BUFFERS=1 is the measurement's other form (DESIGN.md 4d-check):
// one buffer, so a pass is gathered only once the copy before it has left the buffer and copied only once the pass before
// it has been compared.
#ifndef DINT_CHECK_BUFFERS
#define DINT_CHECK_BUFFERS 2
#endif
constexpr size_t kCheckBuffers = DINT_CHECK_BUFFERS;
static_assert(kCheckBuffers == 1 || kCheckBuffers == 2, "the handle has two staging buffers");

namespace {
struct check_pipeline {  // the call's copy stream and events; released with the call
    hipStream_t copy = nullptr;
    hipEvent_t copied[2] = {nullptr, nullptr}, compared[2] = {nullptr, nullptr};
    bool create() {
        if (!hip_ok(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking), "hipStreamCreateWithFlags")) return false;
        for (int k = 0; k != 2; ++k)
            if (!hip_ok(hipEventCreateWithFlags(&copied[k], hipEventDisableTiming), "hipEventCreateWithFlags") ||
                !hip_ok(hipEventCreateWithFlags(&compared[k], hipEventDisableTiming), "hipEventCreateWithFlags"))
                return false;
        return true;
    }
    // the error path once something may be running: both streams waited for, then the status
    int failed(hipStream_t s, int st) const {
        (void)hipStreamSynchronize(copy);
        return stream_failed(s, st);
    }
    ~check_pipeline() {
        for (int k = 0; k != 2; ++k) {
            if (copied[k]) (void)hipEventDestroy(copied[k]);
            if (compared[k]) (void)hipEventDestroy(compared[k]);
        }
        if (copy) (void)hipStreamDestroy(copy);
    }
};

// Walks the blocks of the index in table order: which list a block belongs to, which of the list's blocks it is, the
// global ordinal of the list's first posting.
struct check_cursor {
    const dint_query_index* qi;
    uint32_t list = 0, j = 0;
    uint64_t list_ordinal = 0;
    void settle() {  // on a list that has a block left
        while (list != qi->list_len.size() && j == qi->blocks_of(list)) list_ordinal += qi->list_len[list], ++list, j = 0;
    }
};
// `count` postings of `list` from its position `from` on: words [to, to + count) of a pass's expected docIDs (and freqs)
struct check_segment {
    uint32_t list;
    uint64_t from;
    size_t to, count;
};
}  // namespace

int dint_check_index(dint_query_index* qi, const dint_dict* freqs_dict, const dint_collection_view* view, uint64_t* n_mismatches,
                     dint_index_mismatch* first, void* stream) {
    if (!qi || !view || !n_mismatches) return DINT_ERR_ARG;
    const size_t n_lists = qi->list_len.size(), n_blocks = qi->n_blocks;
    if (view->n_lists != n_lists) return DINT_ERR_ARG;
    if (n_lists && (!view->docs || !view->docs_at || !view->list_len)) return DINT_ERR_ARG;
    if ((freqs_dict != nullptr) != (view->freqs != nullptr) && n_lists) return DINT_ERR_ARG;
    if (freqs_dict && n_lists && !view->freqs_at) return DINT_ERR_ARG;
    if (freqs_dict && (freqs_dict->device != qi->docs->device || freqs_dict->kind != qi->docs->kind)) return DINT_ERR_ARG;
    if (!qi->whole_blocks) return DINT_ERR_ARG;  // (a table whose blocks are not the in-index layout's: no positions to compare at)
    const bool with_freqs = freqs_dict != nullptr && view->freqs != nullptr;
    *n_mismatches = 0;
    if (first) *first = dint_index_mismatch{};

    // lengths, on the host (verify_collection.hpp:18-24): the lowest list of wrong length, and how many there are
    uint64_t wrong_lengths = 0;
    size_t first_wrong_length = n_lists;
    for (size_t l = 0; l != n_lists; ++l)
        if (view->list_len[l] != qi->list_len[l]) {
            if (wrong_lengths++ == 0) first_wrong_length = l;
        }
    auto length_mismatch = [&] {
        dint_index_mismatch m{};
        m.kind = DINT_CHECK_LENGTH, m.list = uint32_t(first_wrong_length);
        m.expected = view->list_len[first_wrong_length], m.got = qi->list_len[first_wrong_length];
        return m;
    };
    if (n_blocks == 0) {
        *n_mismatches = wrong_lengths;
        if (first && wrong_lengths) *first = length_mismatch();
        return DINT_OK;
    }

    std::lock_guard<std::mutex> lock(qi->mutex);
    HIP_TRY(hipSetDevice(qi->docs->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t limit = std::min(size_t(std::min<long long>(opt(DINT_OPT_QUERY_OR_PASS_PAGES), 0x7FFFFFFFll)), kCheckPassPages);
    const size_t pass_pages = std::min(limit, n_blocks);
    constexpr size_t kRecordWords = sizeof(check_page) / 4;
    const size_t pass_words = pass_pages * (kRecordWords + (with_freqs ? 2 : 1) * size_t(kPageSlots));
    // everything the passes need, before the first launch: no buffer is grown (freed) under a pass in flight
    if (qi->stage(2 * kPageSlots * 4) != hipSuccess || !qi->sub.ensure(pass_pages) || !qi->probe.ensure(pass_pages * kPageSlots) ||
        (with_freqs && !qi->fprobe.ensure(pass_pages * kPageSlots)) || !qi->ms_touched.ensure(pass_pages) || !qi->freq_sums.ensure(2) ||
        !qi->expect[0].ensure(pass_words) || !qi->expect[1].ensure(pass_words))
        return DINT_ERR_HIP;
    if (qi->h_expect_cap < pass_words * 4) {
        for (void*& p : qi->h_expect) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
        }
        qi->h_expect_cap = 0;
        for (void*& p : qi->h_expect)
            if (!hip_ok(counted_host_malloc(&p, pass_words * 4), "counted_host_malloc(expected postings)")) return DINT_ERR_HIP;
        qi->h_expect_cap = pass_words * 4;
    }
    check_pipeline pipe;
    if (!pipe.create()) return DINT_ERR_HIP;
    unsigned long long* const d_out = qi->freq_sums.p;  // {postings that differ, the smallest ordinal of one}
    HIP_TRY(hipMemsetAsync(d_out, 0, 8, s));
    HIP_TRY(hipMemsetAsync(d_out + 1, 0xFF, 8, s));

    const uint32_t tb = 256;
    check_cursor at{qi};
    std::vector<check_segment> segments;
    size_t pass = 0;
    for (size_t b0 = 0; b0 != n_blocks; ++pass) {
        const size_t n = std::min(limit, n_blocks - b0);
        const int k = int(pass % kCheckBuffers);
        // the copy that last used this pinned buffer (pass - 2) has left it
        if (pass >= kCheckBuffers && !hip_ok(hipEventSynchronize(pipe.copied[k]), "hipEventSynchronize")) return pipe.failed(s, DINT_ERR_HIP);
        uint32_t* const words = static_cast<uint32_t*>(qi->h_expect[k]);
        check_page* const records = static_cast<check_page*>(qi->h_expect[k]);
        uint32_t* const h_docs = words + n * kRecordWords;
        // records first: a list segment of the pass is consecutive blocks of one list, its postings contiguous in the view.
        // The freqs go behind all the docIDs, so nothing is copied before the pass's postings are counted.
        segments.clear();
        size_t filled = 0;
        for (size_t page = 0; page != n;) {
            at.settle();
            const uint32_t l = at.list;
            const uint32_t blocks = uint32_t(std::min<size_t>(qi->blocks_of(l) - at.j, n - page));
            const uint64_t len = qi->list_len[l], from = uint64_t(at.j) * kPageSlots;
            const bool skip = view->list_len[l] != len;
            const size_t count = skip ? 0 : size_t(std::min<uint64_t>(len, from + uint64_t(blocks) * kPageSlots) - from);
            for (uint32_t j = 0; j != blocks; ++j) {
                check_page& r = records[page + j];
                r.ordinal = at.list_ordinal + from + uint64_t(j) * kPageSlots;
                r.at = uint32_t(filled + size_t(j) * kPageSlots);
                r.n = skip ? 0u : uint32_t(std::min<uint64_t>(kPageSlots, len - from - uint64_t(j) * kPageSlots));
            }
            if (count) segments.push_back({l, from, filled, count});
            filled += count;
            at.j += blocks;
            page += blocks;
        }
        for (const check_segment& g : segments) {
            std::memcpy(h_docs + g.to, view->docs + view->docs_at[g.list] + g.from, g.count * 4);
            if (with_freqs) std::memcpy(h_docs + filled + g.to, view->freqs + view->freqs_at[g.list] + g.from, g.count * 4);
        }
        const size_t words_up = n * kRecordWords + (with_freqs ? 2 : 1) * filled;
        uint32_t* const d_words = qi->expect[k].p;
        // the compare that last used this device buffer (pass - 2) has read it
        if (pass >= kCheckBuffers && !hip_ok(hipStreamWaitEvent(pipe.copy, pipe.compared[k], 0), "hipStreamWaitEvent")) return pipe.failed(s, DINT_ERR_HIP);
        if (!hip_ok(hipMemcpyAsync(d_words, words, words_up * 4, hipMemcpyHostToDevice, pipe.copy), "hipMemcpyAsync(expected postings)") ||
            !hip_ok(hipEventRecord(pipe.copied[k], pipe.copy), "hipEventRecord"))
            return pipe.failed(s, DINT_ERR_HIP);
        hipLaunchKernelGGL(block_ids_kernel, dim3(uint32_t((n + tb - 1) / tb)), dim3(tb), 0, s, uint32_t(b0), uint32_t(n), qi->ms_touched.p);
        const int st = gather_decode_pages(qi, qi->ms_touched.p, nullptr, n, 0, freqs_dict, s);
        if (st != DINT_OK) return pipe.failed(s, st);
        if (!hip_ok(hipStreamWaitEvent(s, pipe.copied[k], 0), "hipStreamWaitEvent")) return pipe.failed(s, DINT_ERR_HIP);
        const uint32_t* const d_docs = d_words + n * kRecordWords;
        hipLaunchKernelGGL(check_pages_kernel, dim3(uint32_t(n)), dim3(kPageSlots), 0, s, reinterpret_cast<const check_page*>(d_words),
                           qi->probe.p, with_freqs ? qi->fprobe.p : nullptr, d_docs, with_freqs ? d_docs + filled : nullptr, d_out);
        if (hipGetLastError() != hipSuccess || !hip_ok(hipEventRecord(pipe.compared[k], s), "hipEventRecord"))
            return pipe.failed(s, DINT_ERR_HIP);
        b0 += n;
    }
    if (!hip_ok(hipMemcpyAsync(qi->h_stage, d_out, 16, hipMemcpyDeviceToHost, s), "hipMemcpyAsync(check results)") ||
        !hip_ok(hipStreamSynchronize(s), "hipStreamSynchronize"))
        return pipe.failed(s, DINT_ERR_HIP);
    const uint64_t wrong_postings = qi->h<uint64_t>(0)[0], key = qi->h<uint64_t>(0)[1];
    *n_mismatches = wrong_lengths + wrong_postings;
    if (!first || *n_mismatches == 0) return DINT_OK;

    // the first posting that differs: its list and position from the ordinal
    size_t l = n_lists;
    uint64_t position = 0;
    if (wrong_postings) {
        uint64_t before = 0;
        for (l = 0; l != n_lists && before + qi->list_len[l] <= key; ++l) before += qi->list_len[l];
        if (l == n_lists) {
            g_hip_error = "dint_check_index: a mismatch beyond the last posting";
            return DINT_ERR_HIP;
        }
        position = key - before;
    }
    if (first_wrong_length < l) {  // (LENGTH before any posting of the list, and a list of wrong length has none compared)
        *first = length_mismatch();
        return DINT_OK;
    }
    // `got`: that one block decoded again, its page brought back
    const uint32_t block = qi->list_first[l] + uint32_t(position / kPageSlots), slot = uint32_t(position % kPageSlots);
    hipLaunchKernelGGL(block_ids_kernel, dim3(1), dim3(tb), 0, s, block, 1u, qi->ms_touched.p);
    const int st = gather_decode_pages(qi, qi->ms_touched.p, nullptr, 1, 0, freqs_dict, s);
    if (st != DINT_OK) return stream_failed(s, st);
    HIP_TRY(hipMemcpyAsync(qi->h_stage, qi->probe.p, kPageSlots * 4, hipMemcpyDeviceToHost, s));
    if (with_freqs) HIP_TRY(hipMemcpyAsync(qi->h(kPageSlots), qi->fprobe.p, kPageSlots * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    dint_index_mismatch m{};
    m.list = uint32_t(l), m.position = position;
    const uint32_t got_doc = qi->h(0)[slot], want_doc = view->docs[view->docs_at[l] + position];
    if (got_doc != want_doc) {  // (DOCID before FREQ: verify_collection.hpp:30-46)
        m.kind = DINT_CHECK_DOCID, m.expected = want_doc, m.got = got_doc;
    } else {
        m.kind = DINT_CHECK_FREQ;
        m.expected = with_freqs ? view->freqs[view->freqs_at[l] + position] : 0;
        m.got = with_freqs ? qi->h(kPageSlots)[slot] : 0;
        if (!with_freqs || m.expected == m.got) {
            g_hip_error = "dint_check_index: the block decoded again holds no mismatch";
            return DINT_ERR_HIP;
        }
    }
    *first = m;
    return DINT_OK;
}
