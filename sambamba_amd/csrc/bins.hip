// bins.hip -- K16: the bin field of BAM records (`sambamba index -c`, `sambamba fixbins`).
//
//   K16a k_check_bins   one lane per record of a batch of sbx_index_bam's pass, next to the index-mode lane of bai_parallel.hpp: the
//                       stored bin of a placed record against binc::expected_bin.  RecDesc::end is not used: it is pos + basesCovered()
//                       only for the records K2 admits (a filter, a selection or a span of zero leave it at pos), so the lane walks
//                       the CIGAR itself.  Mismatches are counted once per wave; the lowest record number among them is kept (atomicMin).
//   K16b k_fix_bins     one lane per record of a batch of sbx_fixbins' read pass, behind the copy of the batch into the resident
//                       store: offset and length of the record for the writer, and the two bytes of the bin stored when they differ.
//                       Every store of a lane lies inside its own record.  On the streamed path (BinFixArgs::bin_out) the records
//                       are read where K1 left them and the bin of a record that changes goes to bin_out for K21 (stream.hip).
//
// Both read 36 bytes + name length + CIGAR per record, scattered by record; K16b writes two bytes of the records it changes.  Next to
// the inflate and record-index kernels of the same pass this is small; NOTHING here has a measured time.
#include "bins.hpp"
#include "bins_core.hpp"
#include "common.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

__global__ __launch_bounds__(kBinThreads) void k_check_bins(const uint8_t* __restrict__ U, const RecDesc* __restrict__ desc,
                                                            const int32_t* __restrict__ rec_ref, uint64_t n, uint64_t rec_base, uint64_t u_end,
                                                            unsigned long long* __restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * kBinThreads + threadIdx.x;
    bool wrong = false;
    if (i < n && rec_ref[i] >= 0 && desc[i].pos >= 0) {
        const uint64_t rec_off = desc[i].rec_off;
        if (rec_off + 36 <= u_end) {
            const uint8_t* p = U + rec_off;
            const uint32_t bs = ld32(p);
            uint32_t want = 0;
            if (record_len_ok(bs, rec_off, u_end) && binc::expected_bin(p, bs, &want)) wrong = want != binc::stored_bin(p);
        }
    }
    const unsigned long long m = __ballot(wrong);
    if (wrong) atomicMin(acc + kBinCheckFirst, (unsigned long long)(rec_base + i));
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(acc + kBinCheckBad, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kBinThreads) void k_fix_bins(BinFixArgs a) {
    __shared__ unsigned long long w_sum[kBinThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kBinThreads + threadIdx.x;
    bool bad = false, changed = false;
    unsigned long long len = 0;
    uint32_t patch = streamc::kNoPatch;
    if (i < a.n) {
        const uint64_t at = a.out_base + i;
        const uint64_t so = (uint64_t)((int64_t)a.desc[i].rec_off + a.store_delta);
        bad = true;
        if (so + 36 <= a.store_end) {
            uint8_t* p = a.store + so;
            const uint32_t bs = ld32(p);
            uint32_t want = 0;
            if (record_len_ok(bs, so, a.store_end) && binc::expected_bin(p, bs, &want)) {
                bad = false;
                len = bs + 4ull;
                changed = want != binc::stored_bin(p);
                if (changed && !a.bin_out) { p[14] = (uint8_t)want; p[15] = (uint8_t)(want >> 8); }
                if (changed) patch = want;
            }
        }
        if (a.bin_out) a.bin_out[i] = patch;             // (K21 writes the two bytes on their way into the window)
        else { a.off[at] = so; a.len[at] = (uint32_t)len; }
    }
    const unsigned long long bytes = block_sum<unsigned long long>(len, w_sum);
    const unsigned long long mb = __ballot(bad), mc = __ballot(changed);
    if ((threadIdx.x & 63u) == 0) {
        if (mb) atomicAdd(a.acc + kBinFixBad, (unsigned long long)__popcll(mb));
        if (mc) atomicAdd(a.acc + kBinFixChanged, (unsigned long long)__popcll(mc));
    }
    if (threadIdx.x == 0 && bytes) atomicAdd(a.acc + kBinFixBytes, bytes);
}

}  // namespace

void launch_check_bins(const uint8_t* d_U, const RecDesc* d_desc, const int32_t* d_rec_ref, uint64_t n, uint64_t rec_base, uint64_t u_end,
                       unsigned long long* d_acc, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_check_bins, dim3(bin_groups(n)), dim3(kBinThreads), 0, stream, d_U, d_desc, d_rec_ref, n, rec_base, u_end, d_acc);
    SBX_HIP(hipGetLastError());
}

void launch_fix_bins(const BinFixArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_fix_bins, dim3(bin_groups(a.n)), dim3(kBinThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
