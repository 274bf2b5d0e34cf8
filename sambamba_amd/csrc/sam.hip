// sam.hip -- K13: the SAM text of `sambamba view` (BamRead.toSam, read.d:695-760) for the entries sbx_view_sam selected.
//
//   K13a k_sam_measure   one lane per entry: the record walker of sam_core.hpp with the sink that only adds lengths up.  The line's
//                        length is stored, the lengths of a workgroup are summed (block_sum) in 64 bits, malformed records are
//                        counted once per wave.  launch_scan64 over the sums and launch_group_offsets (scan.hip) give every line
//                        its 64-bit offset.
//   k_sam_pieces         one lane: cuts the text into pieces of at most `budget` bytes at line ends -- a binary search over the
//                        offsets per piece, a few hundred pieces for a whole genome.
//   K13b k_sam_emit      one lane per entry of a piece: the walker again, with the sink that writes (fmt::RowSink: eight bytes per
//                        store, every store inside the lane's own line).
//
// One lane per entry, for every field: the fixed fields, the CIGAR and the tags are a serial walk anyway, and the two long fields
// are produced eight bytes per store by their lane.  Spreading sequence and qualities over a sub-group of lanes would even out
// lines of different lengths inside a wave; neither layout has been timed, this is the simpler one.
//
// Bytes moved per entry of r record bytes and t text bytes: K13a reads 16 + r (the tags are walked for their lengths; sequence and
// qualities are not touched) and writes 4; the offsets 4 in, 8 out; K13b reads 28 + r and writes t.
#include "common.hpp"
#include "sam.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

__global__ __launch_bounds__(kGroupThreads) void k_sam_measure(SamEntries e, uint32_t* __restrict__ line_len, uint64_t* __restrict__ group_sum,
                                                            unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long w_sum[kGroupThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    uint64_t length = 0;
    bool bad = false, too_long = false;
    if (i < e.n) {
        const uint32_t r = e.perm[i];
        bad = samc::sam_line_length(e.store + e.off[r], e.len[r], e.refs, &length) != samc::kSamOk;
        if (bad) length = 0;
        if (length > 0xFFFFFFFFull) { too_long = true; length = 0; }
        line_len[i] = (uint32_t)length;
    }
    const unsigned long long all = block_sum<unsigned long long>(length, w_sum);
    const unsigned long long mb = __ballot(bad), ml = __ballot(too_long);
    if ((threadIdx.x & 63u) == 0) {
        if (mb) atomicAdd(acc + kSamAccBad, (unsigned long long)__popcll(mb));
        if (ml) atomicAdd(acc + kSamAccTooLong, 1ull);
    }
    if (threadIdx.x == 0) group_sum[blockIdx.x] = all;
}

__global__ void k_sam_pieces(const uint64_t* __restrict__ line_off, uint64_t n, uint64_t budget, uint32_t* __restrict__ first,
                             uint64_t* __restrict__ first_off, uint32_t* __restrict__ n_pieces) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t i = 0;
    uint32_t k = 0;
    while (i < n) {
        if (first) { first[k] = (uint32_t)i; first_off[k] = line_off[i]; }
        ++k;
        // the last line end within the budget; the piece holds line i whatever its length
        const uint64_t base = line_off[i];
        uint64_t lo = i + 1, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo + 1) / 2;
            if (line_off[mid] - base <= budget) lo = mid; else hi = mid - 1;
        }
        i = lo;
    }
    if (first) { first[k] = (uint32_t)n; first_off[k] = n ? line_off[n] : 0ull; }
    *n_pieces = k;
}

__global__ __launch_bounds__(kGroupThreads) void k_sam_emit(SamEntries e, const uint32_t* __restrict__ line_len, const uint64_t* __restrict__ line_off,
                                                         uint64_t i0, uint64_t i1, uint8_t* __restrict__ piece, unsigned long long* __restrict__ acc) {
    const uint64_t i = i0 + (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    bool wrong = false;
    if (i < i1) {
        const uint32_t r = e.perm[i];
        const uint64_t at = line_off[i] - line_off[i0];
        wrong = samc::sam_line_emit(e.store + e.off[r], e.len[r], e.refs, piece + at, line_len[i]) != samc::kSamOk;
    }
    const unsigned long long m = __ballot(wrong);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(acc + kSamAccOverrun, (unsigned long long)__popcll(m));
}

}  // namespace

void launch_sam_measure(const SamEntries& e, uint32_t* d_line_len, uint64_t* d_group_sum, unsigned long long* d_acc, hipStream_t stream) {
    if (!e.n) return;
    hipLaunchKernelGGL(k_sam_measure, dim3(group_count(e.n)), dim3(kGroupThreads), 0, stream, e, d_line_len, d_group_sum, d_acc);
    SBX_HIP(hipGetLastError());
}

void launch_sam_pieces(const uint64_t* d_line_off, uint64_t n, uint64_t budget, uint32_t* d_first, uint64_t* d_first_off, uint32_t* d_n_pieces,
                       hipStream_t stream) {
    hipLaunchKernelGGL(k_sam_pieces, dim3(1), dim3(64), 0, stream, d_line_off, n, budget, d_first, d_first_off, d_n_pieces);
    SBX_HIP(hipGetLastError());
}

void launch_sam_emit(const SamEntries& e, const uint32_t* d_line_len, const uint64_t* d_line_off, uint64_t i0, uint64_t i1, uint8_t* d_piece,
                     unsigned long long* d_acc, hipStream_t stream) {
    if (i1 <= i0) return;
    hipLaunchKernelGGL(k_sam_emit, dim3(group_count(i1 - i0)), dim3(kGroupThreads), 0, stream, e, d_line_len, d_line_off, i0, i1, d_piece, d_acc);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
