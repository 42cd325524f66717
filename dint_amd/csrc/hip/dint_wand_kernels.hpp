// BM25 maxima from the index (wand_data's max_term_weight, reference include/ds2i/wand_data.hpp:18-57, and the same
// maximum per block): DESIGN.md 4d-wand.
//
// The host decodes the index pass by pass into pages (docs and freqs, 256 slots per block) and block_max_weight_kernel
// reduces every page to one float: the largest doc_term_weight(freq, norm_lens[docid]) of the block's postings. Once every
// block has its maximum, list_max_weight_kernel takes the maximum over each list's block range. A maximum of binary32
// values does not depend on the order they are taken in, so both equal the host's sequential std::max bit for bit:
// nothing here is atomic and nothing is ordered. The host's maximum starts at 0.0f and std::max(max, score) keeps `max`
// unless max < score, so a NaN (a norm_len of 0 under a wrapped freq of 0), a negative value or -0.0f never enters it:
// only values > 0.0f do, and those order as their bit patterns do.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dint_kernels.hpp"
#include "dint_query_kernels.hpp"
#include "dint_ranked_query_kernels.hpp"

namespace dint_dev {

// ids[i] = first + i: the consecutive blocks of a pass, as gather_pages_kernel takes them
__global__ void block_ids_kernel(uint32_t first, uint32_t n, uint32_t* ids) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ids[i] = first + i;
}

// what a weight adds to a maximum that starts at 0.0f: its bits if it is > 0.0f, else those of 0.0f
__device__ __forceinline__ uint32_t max_weight_bits(float w) { return w > 0.0f ? __float_as_uint(w) : 0u; }

// the largest of x over the wave, in every lane
__device__ __forceinline__ uint32_t wave_max(uint32_t x) { return readlane(wave_inclusive_max(x), kWave - 1); }

// A workgroup per page of the pass, a thread per slot: page i holds block first + i of the index. One store per block.
__global__ __launch_bounds__(256) void block_max_weight_kernel(const dint_block_ref* blocks, uint32_t first, const uint32_t* docs,
                                                               const uint32_t* freqs, const float* norm_lens, float* block_max_weight) {
    __shared__ uint32_t s_wave[kPageSlots / kWave];
    const uint32_t page = blockIdx.x, slot = threadIdx.x;
    const uint32_t n = blocks[first + page].n;
    uint32_t bits = 0;  // (a slot at or beyond n holds no posting: 0.0f)
    if (slot < n) {
        const uint64_t at = uint64_t(page) * kPageSlots + slot;
        bits = max_weight_bits(bm25_doc_term_weight(float(freqs[at]), bm25_kd(norm_lens[docs[at]])));
    }
    bits = wave_max(bits);
    if ((slot & (kWave - 1)) == 0) s_wave[slot / kWave] = bits;
    __syncthreads();
    if (slot != 0) return;
    for (uint32_t w = 1; w != kPageSlots / kWave; ++w) bits = s_wave[w] > bits ? s_wave[w] : bits;
    block_max_weight[first + page] = __uint_as_float(bits);
}

// A wave per list, striding over its blocks (the longest lists have 10^5 of them): max_term_weight[t] = the largest
// block maximum of list t, 0.0f for a list without a block. The block maxima are >= 0.0f and no NaN (the kernel above).
__global__ __launch_bounds__(256) void list_max_weight_kernel(const uint32_t* list_first, uint32_t n_lists, const float* block_max_weight,
                                                              float* max_term_weight) {
    const uint32_t t = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    if (t >= n_lists) return;  // (whole waves)
    uint32_t bits = 0;
    for (uint32_t b = list_first[t] + lane; b < list_first[t + 1]; b += kWave) {
        const uint32_t x = __float_as_uint(block_max_weight[b]);
        bits = x > bits ? x : bits;
    }
    bits = wave_max(bits);
    if (lane == 0) max_term_weight[t] = __uint_as_float(bits);
}

}  // namespace dint_dev
