// The pure lookups of the query kernels ("Shared device primitives"): is docID d in a list, and where?
// Plain C++ over arrays — no HIP builtin, nothing included but <cstdint> — so tests/test_query_lookup_cpu.py compiles
// this file alone with g++ and holds it to numpy.searchsorted.
#pragma once
#include <cstdint>

namespace dint_dev {

constexpr uint32_t kPageSlots = 256;    // one block per page
constexpr uint32_t kAbsent = ~0u;     // not a position in a page

// first index in [0, n) with a[i] >= key (n if none)
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* a, uint32_t n, uint32_t key) {
    uint32_t lo = 0, len = n;
    while (len) {
        const uint32_t half = len >> 1;
        const bool right = a[lo + half] < key;
        lo = right ? lo + half + 1 : lo;
        len = right ? len - half - 1 : half;
    }
    return lo;
}

// The position of d among the first n slots of a decoded page (ascending docIDs), or kAbsent. The slots past n are
// padding and are never read.
__device__ __forceinline__ uint32_t find_in_page(const uint32_t* page, uint32_t n, uint32_t d) {
    const uint32_t pos = lower_bound_u32(page, n, d);
    return pos < n && page[pos] == d ? pos : kAbsent;  // (<, not !=: it tells the compiler that a position is never kAbsent)
}

// next_geq's block-max search: the position in [0, nb] of the first block of the list (blocks fb .. fb + nb of the
// index) whose last docID is >= d. nb: d is past the list's last docID (always so for an empty list, nb == 0).
__device__ __forceinline__ uint32_t list_block_of(const uint32_t* block_max, uint32_t fb, uint32_t nb, uint32_t d) {
    return lower_bound_u32(block_max + fb, nb, d);
}

// The blocks of a list that can hold a docID of [lo, hi): the positions [p0, p1) of its nb blocks, whose last docIDs are
// block_max[0 .. nb) — p0 the first block that ends at or past lo, p1 one past the first block that ends at or past
// hi - 1 (a block past that one begins past hi - 1). lo >= hi, or a list that ends before lo: no block (p0 == p1). Every
// posting d of the list with lo <= d < hi lies in a block of [p0, p1); only blocks p0 and p1 - 1 may also hold postings
// outside the range.
// constexpr, and so callable from the host's planning as from a kernel: the ranged calls plan their pages on the host, over
// the handle's own copy of the maxima (lower_bound_u32 above is the kernels' alone).
struct block_span {
    uint32_t p0, p1;
    constexpr uint32_t size() const { return p1 - p0; }
};
constexpr uint32_t first_block_reaching(const uint32_t* block_max, uint32_t nb, uint32_t d) {
    uint32_t at = 0, len = nb;
    while (len) {
        const uint32_t half = len >> 1;
        const bool right = block_max[at + half] < d;
        at = right ? at + half + 1 : at;
        len = right ? len - half - 1 : half;
    }
    return at;
}
constexpr block_span list_blocks_in_range(const uint32_t* block_max, uint32_t nb, uint32_t lo, uint32_t hi) {
    if (lo >= hi) return {0, 0};
    const uint32_t p0 = first_block_reaching(block_max, nb, lo);
    const uint32_t last = first_block_reaching(block_max, nb, hi - 1);
    return {p0, last < nb ? last + 1 : nb};
}

// Is d in the list, and where? The list's blocks lie decoded in pages of `docs`, block position pos in page
// page_of(pos) (asked only for a block d can be in). -> the page's first slot in docs and d's position in the page (its
// freq is at the same slot of the freqs pages), or hit == kAbsent. blocks[b].n: the docIDs of block b of the index.
struct posting {
    uint64_t page;
    uint32_t hit;
    __device__ __forceinline__ bool held() const { return hit != kAbsent; }
    __device__ __forceinline__ uint64_t slot() const { return page + hit; }
};
template <class Block, class PageOf>
__device__ __forceinline__ posting find_posting(const uint32_t* block_max, const Block* blocks, uint32_t fb, uint32_t nb,
                                                const uint32_t* docs, uint32_t d, PageOf page_of) {
    const uint32_t pos = list_block_of(block_max, fb, nb, d);
    if (pos == nb) return {0, kAbsent};
    const uint32_t n = blocks[fb + pos].n;
    const uint64_t page = uint64_t(page_of(pos)) * kPageSlots;
    return {page, find_in_page(docs + page, n, d)};
}

}  // namespace dint_dev
