// scan.hip -- the device scans every command shares (scan.hpp).
#include "scan.hpp"

#include "common.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// ---- scan of the per-block counts (single workgroup, 3 phases; n_blocks is ~1e5..1e6) -----------
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_count_scan(const uint32_t* __restrict__ count, uint32_t n,
                                                              uint64_t* __restrict__ base) {
    // tiles of 4 x kScanThreads counts, four consecutive ones per thread (one 16-byte load, coalesced); a shuffle scan inside the
    // wavefront, the sixteen wave totals through LDS, the running sum carried from tile to tile.  (Until round 6 every thread summed its
    // own stretch of n / 1024 counts, one strided load at a time, around a Hillis-Steele scan of the 1024 partials: 58 us for the 32 k
    // chunk lengths of a piece of K6's text, a sixth of what formatting the piece took.)
    __shared__ uint64_t wtot[kScanThreads / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
    uint64_t carry = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 4u * kScanThreads) {
        const uint32_t i = i0 + 4u * t;
        uint32_t v[4] = {0, 0, 0, 0};
        if (i + 4u <= n) {
            const uint4 q = *(const uint4*)(count + i);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (uint32_t k = 0; k < 4u; ++k) if (i + k < n) v[k] = count[i + k];
        }
        const uint64_t s = (uint64_t)v[0] + v[1] + v[2] + v[3];
        uint64_t incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t o = (uint64_t)__shfl_up((unsigned long long)incl, d, 64);
            if ((int)lane >= d) incl += o;
        }
        if (lane == 63) wtot[wv] = incl;
        __syncthreads();
        uint64_t before = carry, tile = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
            const uint64_t x = wtot[w];
            if (w < wv) before += x;
            tile += x;
        }
        uint64_t run = before + incl - s;
#pragma unroll
        for (uint32_t k = 0; k < 4u; ++k) {
            if (i + k < n) base[i + k] = run;
            run += v[k];
        }
        carry += tile;
        __syncthreads();
    }
    if (t == 0) base[n] = carry;
}

// in place: x[i] = first + sum of x[j], j < i, for i in [0, m]; one workgroup
__global__ __launch_bounds__(1024) void k_scan64(uint64_t* __restrict__ x, uint64_t m, uint64_t first) {
    __shared__ uint64_t wsum[1024 / 64];
    uint64_t carry = first;
    for (uint64_t i0 = 0; i0 < m; i0 += 1024) {
        const uint64_t i = i0 + threadIdx.x;
        const uint64_t v = i < m ? x[i] : 0;
        uint64_t total;
        const uint64_t ex = block_exclusive(v, wsum, &total);
        if (i < m) x[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) x[m] = carry;
}

// ---- lengths through a permutation (or none), kLenTile per workgroup ----
constexpr uint32_t kLenThreads = 256, kLenItems = kLenTile / kLenThreads;

__global__ __launch_bounds__(kLenThreads) void k_len_tile_sum(const uint32_t* __restrict__ len, const uint32_t* __restrict__ perm, uint64_t n,
                                                              uint64_t* __restrict__ tile_sum) {
    __shared__ uint64_t wsum[kLenThreads / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kLenTile + (uint64_t)threadIdx.x * kLenItems;
    uint64_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLenItems; ++k) if (i0 + k < n) s += len[perm ? perm[i0 + k] : i0 + k];
    s = block_sum(s, wsum);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = s;
}

__global__ __launch_bounds__(kLenThreads) void k_len_apply(const uint32_t* __restrict__ len, const uint32_t* __restrict__ perm, uint64_t n,
                                                           const uint64_t* __restrict__ tile_base, uint64_t* __restrict__ out_off) {
    __shared__ uint64_t wsum[kLenThreads / 64];
    const uint64_t i0 = (uint64_t)blockIdx.x * kLenTile + (uint64_t)threadIdx.x * kLenItems;
    uint32_t l[kLenItems];
    uint64_t s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLenItems; ++k) { l[k] = i0 + k < n ? len[perm ? perm[i0 + k] : i0 + k] : 0u; s += l[k]; }
    uint64_t total;
    uint64_t run = tile_base[blockIdx.x] + block_exclusive(s, wsum, &total);
#pragma unroll
    for (uint32_t k = 0; k < kLenItems; ++k) {
        if (i0 + k < n) out_off[i0 + k] = run;
        run += l[k];
        if (i0 + k + 1 == n) out_off[n] = run;
    }
}

// ---- lengths whose workgroup sums are scanned already ----
__global__ __launch_bounds__(kGroupThreads) void k_group_offsets(const uint32_t* __restrict__ len, const uint64_t* __restrict__ group_base,
                                                                uint64_t n, uint64_t first, uint64_t* __restrict__ off) {
    __shared__ uint64_t w_sum[kGroupThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    uint64_t all;
    const uint64_t before = block_exclusive<uint64_t>(i < n ? len[i] : 0u, w_sum, &all);
    const uint64_t base = first + group_base[blockIdx.x];
    if (i < n) off[i] = base + before;
    if (i + 1 == n) off[n] = base + all;
}

// d[i] = v + step * i
__global__ __launch_bounds__(256) void k_fill32(uint32_t* __restrict__ d, uint32_t v, uint32_t step, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) d[i] = v + step * (uint32_t)i;
}

void fill32(uint32_t* d, uint32_t v, uint32_t step, uint64_t n, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_fill32, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d, v, step, n);
    SBX_HIP(hipGetLastError());
}

}  // namespace

void launch_count_scan(const uint32_t* d_count, uint32_t n, uint64_t* d_base, hipStream_t stream) {
    hipLaunchKernelGGL(k_count_scan, dim3(1), dim3(kScanThreads), 0, stream, d_count, n, d_base);
    SBX_HIP(hipGetLastError());
}

void launch_scan64(uint64_t* d_x, uint64_t m, uint64_t first, hipStream_t stream) {
    hipLaunchKernelGGL(k_scan64, dim3(1), dim3(1024), 0, stream, d_x, m, first);
    SBX_HIP(hipGetLastError());
}

void launch_sorted_offsets(const uint32_t* d_len, const uint32_t* d_perm, uint64_t n, uint64_t first, uint64_t* d_tile_sum, uint64_t* d_out_off,
                           hipStream_t stream) {
    if (!n) return;
    const uint32_t tiles = (uint32_t)len_tiles(n);
    hipLaunchKernelGGL(k_len_tile_sum, dim3(tiles), dim3(kLenThreads), 0, stream, d_len, d_perm, n, d_tile_sum);
    SBX_HIP(hipGetLastError());
    launch_scan64(d_tile_sum, tiles, first, stream);
    hipLaunchKernelGGL(k_len_apply, dim3(tiles), dim3(kLenThreads), 0, stream, d_len, d_perm, n, d_tile_sum, d_out_off);
    SBX_HIP(hipGetLastError());
}

void launch_group_offsets(const uint32_t* d_len, const uint64_t* d_group_base, uint64_t n, uint64_t first, uint64_t* d_off, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_group_offsets, dim3(group_count(n)), dim3(kGroupThreads), 0, stream, d_len, d_group_base, n, first, d_off);
    SBX_HIP(hipGetLastError());
}

void launch_iota(uint32_t* d_val, uint64_t n, hipStream_t stream) { fill32(d_val, 0u, 1u, n, stream); }
void launch_fill32(uint32_t* d, uint32_t v, uint64_t n, hipStream_t stream) { fill32(d, v, 0u, n, stream); }

}  // namespace sbx
