// lines.hip -- K15a: where the lines of a chunk of text start.
//
//   k_count_newlines  one lane per 16 bytes of text, one 16-byte load: the '\n' bytes among them as a 16-bit mask (a zero-byte
//   k_line_starts     test on the four words xor 0x0A0A0A0A), popcount, block_sum per 4 KiB tile; launch_scan64 (scan.hip) over the
//                     tiles; then the same loads and masks again, block_exclusive, and every lane stores the starts of the lines
//                     behind its '\n' bytes.
#include "common.hpp"
#include "lines.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// bit k: byte k of the lane's sixteen is a '\n' of the text (bytes at or behind `size` do not count)
__device__ __forceinline__ uint32_t newline_mask(const TextChunk& t, uint64_t at) {
    if (at >= t.size) return 0u;
    const uint4 v = *(const uint4*)(t.text + at);              // (16-byte aligned; the buffer is readable to the next multiple of 16)
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t x = w[j] ^ 0x0A0A0A0Au;
        const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte of x that is zero, exactly
        m |= (((z >> 7) & 1u) | ((z >> 14) & 2u) | ((z >> 21) & 4u) | ((z >> 28) & 8u)) << (4u * j);
    }
    const uint64_t left = t.size - at;
    return left >= 16u ? m : m & ((1u << (uint32_t)left) - 1u);
}

__global__ __launch_bounds__(kGroupThreads) void k_count_newlines(TextChunk t, uint64_t* __restrict__ tile_sum) {
    __shared__ uint32_t w_sum[kGroupThreads / 64];
    const uint64_t at = ((uint64_t)blockIdx.x * kGroupThreads + threadIdx.x) * kLineLaneBytes;
    const uint32_t all = block_sum<uint32_t>((uint32_t)__popc(newline_mask(t, at)), w_sum);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

__global__ __launch_bounds__(kGroupThreads) void k_line_starts(TextChunk t, const uint64_t* __restrict__ tile_base, uint64_t* __restrict__ line_start) {
    __shared__ uint32_t w_sum[kGroupThreads / 64];
    const uint64_t at = ((uint64_t)blockIdx.x * kGroupThreads + threadIdx.x) * kLineLaneBytes;
    uint32_t m = newline_mask(t, at);
    uint32_t all;
    uint64_t k = tile_base[blockIdx.x] + block_exclusive<uint32_t>((uint32_t)__popc(m), w_sum, &all) + 1u;      // (line 0 starts at byte 0)
    if (at == 0) line_start[0] = 0;
    for (; m; m &= m - 1u) line_start[k++] = at + (uint32_t)__builtin_ctz(m) + 1u;
}

}  // namespace

void launch_count_newlines(const TextChunk& t, uint64_t* d_tile_sum, hipStream_t stream) {
    if (!t.size) return;
    hipLaunchKernelGGL(k_count_newlines, dim3(text_tiles(t.size)), dim3(kGroupThreads), 0, stream, t, d_tile_sum);
    SBX_HIP(hipGetLastError());
}

void launch_line_starts(const TextChunk& t, const uint64_t* d_tile_base, uint64_t* d_line_start, hipStream_t stream) {
    if (!t.size) return;
    hipLaunchKernelGGL(k_line_starts, dim3(text_tiles(t.size)), dim3(kGroupThreads), 0, stream, t, d_tile_base, d_line_start);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
