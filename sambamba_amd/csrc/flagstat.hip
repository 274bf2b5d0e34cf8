// flagstat.hip -- K8: the counters of `sambamba flagstat` (computeFlagStatistics, sambamba/flagstat.d:31-58) over the described
// records of a batch.
//
// A record needs four fields: flag and mapq from its descriptor (index.hip describe), refID from rec_ref and next_refID from the
// fixed part of the record in U (block_size, refID, pos, bin_mq_nl, flag_nc, l_seq, next_refID: bytes 24..27 behind rec_off).
// The 13 counters of the reference, each split by failed = flag & 0x200, are 26 predicates of a record.  A wave tests 64 records at
// a time: per predicate one __ballot, and __popcll of the mask and of its intersection with the QC-failed mask give the two counts --
// wave-uniform numbers, kept in scalar registers across the grid-stride loop.  The waves of a block add theirs through LDS and the
// block makes one 64-bit atomicAdd per non-zero counter into the 26-word result (the layout of sbx_flagstat_counts), which
// accumulates over the batches of a file and is read back once.  Integer atomics: the result does not depend on the order of arrival.
#include "common.hpp"
#include "flagstat.hpp"

namespace sbx {

namespace {

constexpr int kFsThreads = 256;
constexpr int kFsWaves = kFsThreads / 64;
constexpr uint32_t kFsMaxBlocks = 2048;

// field order of sbx_flagstat_counts (flagstat.d:131-143); counter k of failed f is word 2 * k + f
enum { kReads, kSecondary, kSupplementary, kDup, kMapped, kPairAll, kFirst, kSecond, kPairGood, kPairMap, kSingle, kDiffChr,
       kDiffHigh, kFsCounters };

__global__ __launch_bounds__(kFsThreads) void k_flagstat(const uint8_t* __restrict__ U, const RecDesc* __restrict__ desc,
                                                          const int32_t* __restrict__ rec_ref, uint64_t n,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ unsigned long long part[kFsWaves][2 * kFsCounters];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t c[2 * kFsCounters];
#pragma unroll
    for (int k = 0; k < 2 * kFsCounters; ++k) c[k] = 0;
    // the loop bound is the wave's first record, so every wave runs whole iterations and its ballots see all 64 lanes
    const uint64_t stride = (uint64_t)gridDim.x * kFsThreads;
    for (uint64_t w0 = (uint64_t)blockIdx.x * kFsThreads + wave * 64; w0 < n; w0 += stride) {
        const uint64_t i = w0 + lane;
        const bool live = i < n;
        uint32_t flag = 0, mapq = 0;
        int32_t ref = 0, mate_ref = 0;
        if (live) {
            const RecDesc d = desc[i];
            flag = d.flag;
            mapq = d.mapq;
            ref = rec_ref[i];
            __builtin_memcpy(&mate_ref, U + d.rec_off + 24, 4);       // next_refID (records start at any byte)
        }
        const bool unmapped = flag & 0x4, mate_unmapped = flag & 0x8;
        // the if / else-if chain of flagstat.d:40-57: secondary, else supplementary, else paired
        const bool secondary = flag & 0x100, supplementary = !secondary && (flag & 0x800);
        const bool paired = !secondary && !(flag & 0x800) && (flag & 0x1);
        const bool pair_map = paired && !unmapped && !mate_unmapped;
        const bool diff_chr = pair_map && ref != mate_ref;
        const unsigned long long failed = __ballot(live && (flag & 0x200));
        const unsigned long long m[kFsCounters] = {
            __ballot(live),
            __ballot(live && secondary),
            __ballot(live && supplementary),
            __ballot(live && (flag & 0x400)),
            __ballot(live && !unmapped),
            __ballot(live && paired),
            __ballot(live && paired && (flag & 0x40)),
            __ballot(live && paired && (flag & 0x80)),
            __ballot(live && paired && (flag & 0x2) && !unmapped),
            __ballot(live && pair_map),
            __ballot(live && paired && mate_unmapped && !unmapped),
            __ballot(live && diff_chr),
            __ballot(live && diff_chr && mapq >= 5),
        };
#pragma unroll
        for (int k = 0; k < kFsCounters; ++k) {
            c[2 * k] += (uint64_t)__popcll(m[k] & ~failed);
            c[2 * k + 1] += (uint64_t)__popcll(m[k] & failed);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 2 * kFsCounters; ++k) part[wave][k] = c[k];
    }
    __syncthreads();
    if (threadIdx.x < 2 * kFsCounters) {
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kFsWaves; ++w) v += part[w][threadIdx.x];
        if (v) atomicAdd(counts + threadIdx.x, v);
    }
}

}  // namespace

void launch_flagstat(const uint8_t* d_U, const RecDesc* d_desc, const int32_t* d_rec_ref, uint64_t n_records, unsigned long long* d_counts,
                     hipStream_t stream) {
    if (!n_records) return;
    const uint64_t want = (n_records + kFsThreads - 1) / kFsThreads;
    const uint32_t blocks = (uint32_t)(want < kFsMaxBlocks ? want : kFsMaxBlocks);
    hipLaunchKernelGGL(k_flagstat, dim3(blocks), dim3(kFsThreads), 0, stream, d_U, d_desc, d_rec_ref, n_records, d_counts);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
