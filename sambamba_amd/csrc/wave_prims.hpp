// wave_prims.hpp -- the wave and workgroup idioms the kernels of the resident-store commands and of the text commands share.  Included by
// scan.hip, lines.hip, sort.hip (K9), markdup.hip (K10), merge.hip (K11), view.hip (K12), sam.hip (K13), namesort.hip (K14), samparse.hip
// (K15), bins.hip (K16), fasta.hip (K17) and slice.hip (K18).  (The depth path -- inflate, index, depth, reduce, mates, format, deflate, flagstat -- keeps
// private helpers with similar names and does not include this.)  A wave is 64 lanes; a workgroup a whole number of waves, its threads
// numbered by threadIdx.x.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace sbx {

// the lanes of the wave in front of this one
__device__ __forceinline__ uint64_t lanemask_lt() { return (1ull << (threadIdx.x & 63u)) - 1ull; }

// ---- xor-butterfly reductions over the 64 lanes; the result is valid in every lane ----
template <class T>
using shfl_t = std::conditional_t<sizeof(T) == 8, unsigned long long, unsigned int>;

template <class T, class Op>
__device__ __forceinline__ T wave_reduce(T v, Op op) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = op(v, (T)__shfl_xor((shfl_t<T>)v, d, 64));
    return v;
}
template <class T> __device__ __forceinline__ T wave_sum(T v) { return wave_reduce(v, [](T a, T b) { return a + b; }); }
template <class T> __device__ __forceinline__ T wave_min(T v) { return wave_reduce(v, [](T a, T b) { return b < a ? b : a; }); }
template <class T> __device__ __forceinline__ T wave_max(T v) { return wave_reduce(v, [](T a, T b) { return b > a ? b : a; }); }
__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) { return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return a | b; }); }
__device__ __forceinline__ unsigned long long wave_and(unsigned long long v) { return wave_reduce(v, [](unsigned long long a, unsigned long long b) { return a & b; }); }

// inclusive prefix sum over the lanes of the wave (uint32_t or uint64_t): the __shfl_up ladder
template <class T>
__device__ __forceinline__ T wave_inclusive(T v) {
    const int lane = (int)(threadIdx.x & 63u);
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = (T)__shfl_up((shfl_t<T>)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// ---- over the threads of a workgroup.  wsum / wcnt: an LDS row of blockDim.x / 64 words, one per wave.  Every thread of the
// workgroup must make the call: each contains __syncthreads(). ----

// sum of the values of the workgroup's threads; valid in every thread
template <class T>
__device__ __forceinline__ T block_sum(T v, T* wsum) {
    v = wave_sum(v);
    if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = 0;
    for (uint32_t w = 0; w < blockDim.x / 64; ++w) s += wsum[w];
    __syncthreads();
    return s;
}

// exclusive prefix of v over the workgroup's threads (thread order); *total receives the sum
template <class T>
__device__ __forceinline__ T block_exclusive(T v, T* wsum, T* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive(v);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
    for (uint32_t w = 0; w < blockDim.x / 64; ++w) { const T x = wsum[w]; if (w < wave) before += x; all += x; }
    __syncthreads();
    *total = all;
    return before + incl - v;
}

// File-order compaction: how many threads of the workgroup with `keep` set come before this one -- ballot, popcount into the wave's
// word of wcnt (LDS, one word per wave of the workgroup), the words of the waves in front, popcount below the own lane.  *total
// (optional) receives the workgroup's number of kept threads.  One __syncthreads(): every thread of the workgroup must make the
// call, also those that keep nothing, and wcnt must not be written again before the workgroup has passed another barrier.
template <uint32_t kWaves>
__device__ __forceinline__ uint32_t block_rank_of_kept(bool keep, uint32_t (&wcnt)[kWaves], uint32_t* total = nullptr) {
    const uint32_t wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63u) == 0) wcnt[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0;
    for (uint32_t w = 0; w < wave; ++w) before += wcnt[w];
    if (total) {
        uint32_t all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) all += wcnt[w];
        *total = all;
    }
    return before + (uint32_t)__popcll(m & lanemask_lt());
}

// ---- bytes of records: both ends at any byte address ----
__device__ __forceinline__ uint32_t ld32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);                  // (records start at any byte; gfx950 takes global loads at any byte address)
    return v;
}

constexpr uint32_t kCopyGroup = 16;              // lanes that move one record
struct __attribute__((packed, aligned(1))) Bytes16 { uint32_t w[4]; };

// nbytes from src to dst by the sixteen lanes of a record (lane_in_group = 0 .. 15): the destination is brought to a 16-byte
// boundary with a head of single bytes, the body moves 16 bytes per lane (aligned store, unaligned load), the tail is single bytes.
__device__ __forceinline__ void copy_span16(uint8_t* dst, const uint8_t* src, uint64_t nbytes, uint32_t lane_in_group) {
    const uint32_t l = lane_in_group;
    const uint32_t head = (uint32_t)((16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u);
    const uint32_t h = head < nbytes ? head : (uint32_t)nbytes;
    if (l < h) dst[l] = src[l];
    src += h; dst += h; nbytes -= h;
    const uint64_t chunks = nbytes >> 4;
    for (uint64_t c = l; c < chunks; c += kCopyGroup) {
        const Bytes16 x = *(const Bytes16*)(src + 16 * c);
        *(uint4*)(dst + 16 * c) = uint4{x.w[0], x.w[1], x.w[2], x.w[3]};
    }
    const uint32_t tail = (uint32_t)(nbytes & 15u);
    if (l < tail) dst[16 * chunks + l] = src[16 * chunks + l];
}

// ---- the frame of a record at offset rec_off of a batch whose inflated bytes end at u_end ----
// the light check: block_size bs is one a record can have, and the record ends inside the batch
__device__ __forceinline__ bool record_len_ok(uint32_t bs, uint64_t rec_off, uint64_t u_end) {
    return !(bs < 32u || bs > 0x7FFFFFF0u || rec_off + 4ull + bs > u_end);
}

struct RecordFrame {
    uint32_t bs, l_name, n_cigar, flag;
    int32_t ref, pos, l_seq, next_ref;
    uint64_t fixed;                              // bytes behind block_size up to the aux fields: 32 + name + CIGAR + sequence + qualities
};
// The full check: reads the fixed part (not a byte of it unless its 36 bytes lie inside the batch) and returns false when a length
// the record states contradicts its block_size or the batch, or its reference id is outside [-1, n_ref).  Only after `true` may a
// byte behind the fixed part be read, and only up to 4 + bs.
__device__ __forceinline__ bool read_record_frame(const uint8_t* U, uint64_t rec_off, uint64_t u_end, int32_t n_ref, RecordFrame* f) {
    if (rec_off + 36 > u_end) return false;
    const uint8_t* p = U + rec_off;
    f->bs = ld32(p);
    f->ref = (int32_t)ld32(p + 4);
    f->pos = (int32_t)ld32(p + 8);
    f->l_name = p[12];
    const uint32_t fnc = ld32(p + 16);
    f->n_cigar = fnc & 0xFFFFu;
    f->flag = fnc >> 16;
    f->l_seq = (int32_t)ld32(p + 20);
    f->next_ref = (int32_t)ld32(p + 24);
    const uint64_t seq = f->l_seq < 0 ? 0 : (uint64_t)f->l_seq;
    f->fixed = 32 + (uint64_t)f->l_name + 4ull * f->n_cigar + (seq + 1) / 2 + seq;
    return record_len_ok(f->bs, rec_off, u_end) && f->l_seq >= 0 && f->fixed <= f->bs && f->ref >= -1 && f->ref < n_ref;
}

}  // namespace sbx
