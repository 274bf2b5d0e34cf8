// valid.hip -- K19: which records of a batch are valid, and why not (`sambamba view -v`, `sbx-validate`).
//
//   K19 k_valid_masks   one lane per described record, a grid-stride loop of whole waves (the shape of K8): the lane runs
//                       validc::record_mask (valid_core.hpp) over its record in U -- fixed part, name, CIGAR, qualities (eight bytes
//                       per load) and tags, every read checked against the record's block_size and the end of the batch -- and
//                       stores the 16-bit mask.  Per class one __ballot per turn; the popcounts are wave-uniform and stay in scalar
//                       registers across the loop.  The waves of a workgroup add their eleven counters through LDS and the workgroup
//                       makes one 64-bit atomicAdd per non-zero counter, plus one atomicMin with the lowest ordinal of its invalid
//                       records: integer atomics, the result does not depend on the order of arrival.
//
// Bytes read per record: 8 of its descriptor (a 32-byte stride, so the whole descriptor line is fetched) and the record without its
// packed sequence -- 36 + l_read_name + 4 n_cigar + l_seq + the tags; (l_seq + 1) / 2 bytes are skipped.  For a 100-base read with a
// 20-byte name, one CIGAR operation and 40 bytes of tags that is 200 of 250 bytes, 0.8 of the inflated stream; counted in 128-byte
// lines it is all of it, since the skipped 50 bytes sit in the middle of the record.  The roof is therefore one read of the
// inflated batch.  The lanes of a wave read 64 different records, so a load instruction touches up to 64 lines: the kernel is
// bound by the latency of those scattered loads, not by that roof (one run on the chr1 30x file: 31.2 ms for 49.8 M records and
// 14.11 GB inflated).
#include "common.hpp"
#include "valid.hpp"

namespace sbx {

namespace {

constexpr int kVdThreads = 256;
constexpr int kVdWaves = kVdThreads / 64;
constexpr uint32_t kVdMaxBlocks = 4096;
constexpr int kVdCounters = validc::kClasses + 1;      // the classes, then the invalid records

__global__ __launch_bounds__(kVdThreads) void k_valid_masks(ValidArgs a) {
    __shared__ unsigned long long part[kVdWaves][kVdCounters];
    __shared__ unsigned long long first_of[kVdWaves];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t c[kVdCounters];
#pragma unroll
    for (int k = 0; k < kVdCounters; ++k) c[k] = 0;
    unsigned long long first = kValidNone;
    // the loop bound is the wave's first record, so every wave runs whole iterations and its ballots see all 64 lanes
    const uint64_t stride = (uint64_t)gridDim.x * kVdThreads;
    for (uint64_t w0 = (uint64_t)blockIdx.x * kVdThreads + wave * 64; w0 < a.n; w0 += stride) {
        const uint64_t i = w0 + lane;
        uint32_t m = 0;
        if (i < a.n) {
            const uint64_t rec_off = a.desc[i].rec_off;
            m = rec_off < a.u_end ? validc::record_mask(a.U + rec_off, a.u_end - rec_off) : (uint32_t)validc::kMalformed;
            if (a.mask) a.mask[i] = (uint16_t)m;
        }
        const unsigned long long bad = __ballot(m != 0);
        if (bad) {                                           // (wave-uniform)
#pragma unroll
            for (int k = 0; k < validc::kClasses; ++k) c[k] += (uint64_t)__popcll(__ballot((m >> k) & 1u));
            c[validc::kClasses] += (uint64_t)__popcll(bad);
            // file order: the first turn with an invalid record holds the wave's lowest one
            if (first == kValidNone) first = a.rec_base + w0 + (uint64_t)(__ffsll((long long)bad) - 1);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kVdCounters; ++k) part[wave][k] = c[k];
        first_of[wave] = first;
    }
    __syncthreads();
    if (threadIdx.x < kVdCounters) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kVdWaves; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(a.acc + threadIdx.x, v);
    } else if (threadIdx.x == 64) {
        unsigned long long f = kValidNone;
#pragma unroll
        for (int w = 0; w < kVdWaves; ++w) f = first_of[w] < f ? first_of[w] : f;
        if (f != kValidNone) atomicMin(a.acc + kValidAccFirst, f);
    }
}

}  // namespace

void launch_valid_masks(const ValidArgs& a, hipStream_t stream) {
    if (!a.n) return;
    const uint64_t want = (a.n + kVdThreads - 1) / kVdThreads;
    const uint32_t blocks = (uint32_t)(want < kVdMaxBlocks ? want : kVdMaxBlocks);
    hipLaunchKernelGGL(k_valid_masks, dim3(blocks), dim3(kVdThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
