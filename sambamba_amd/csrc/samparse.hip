// samparse.hip -- K15: the lines of a chunk of SAM text (`sambamba view -S -f bam`, parseAlignmentLine of BioD's sam_alignment.rl)
// turned into BAM records in the resident record store.
//
//   K15a k_count_newlines  one lane per 16 bytes of text, one 16-byte load: the '\n' bytes among them as a 16-bit mask (a zero-byte
//        k_line_starts     test on the four words xor 0x0A0A0A0A), popcount, block_sum per 4 KiB tile; import_scan64 over the tiles;
//                          then the same loads and masks again, block_exclusive, and every lane stores the starts of the lines
//                          behind its '\n' bytes.
//   K15b k_import_measure  one lane per line: the line walker of samparse_core.hpp with the sink that only adds lengths up.  The
//                          record's length is stored, the lengths of a workgroup are summed, lines outside the grammar are counted
//                          once per wave and the lowest line number among them is kept (atomicMin).
//   k_import_offsets       the same lanes: 64-bit store offset of every record = fill of the store + scanned base of the workgroup
//                          + block_exclusive.
//   K15c k_import_emit     one lane per line: the walker again, with the sink that writes (fmt::RowSink: eight bytes per store,
//                          every store inside the lane's own record).
//
// One lane per line, for every field, as K13 has it in the other direction: the fields are a serial walk, and the two long ones --
// sequence and qualities -- are produced eight bytes per store by their lane.  The bound this sits under: the text is
// read twice (K15a twice in 16-byte loads that coalesce; K15b and K15c byte by byte, one scattered stream per lane), the record
// bytes are written once.  NOTHING here has a measured time.
#include "common.hpp"
#include "samparse.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// bit k: byte k of the lane's sixteen is a '\n' of the text (bytes at or behind `size` do not count)
__device__ __forceinline__ uint32_t newline_mask(const ImportText& t, uint64_t at) {
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

__global__ __launch_bounds__(kImportThreads) void k_count_newlines(ImportText t, uint64_t* __restrict__ tile_sum) {
    __shared__ uint32_t w_sum[kImportThreads / 64];
    const uint64_t at = ((uint64_t)blockIdx.x * kImportThreads + threadIdx.x) * kImportLaneBytes;
    const uint32_t all = block_sum<uint32_t>((uint32_t)__popc(newline_mask(t, at)), w_sum);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = all;
}

// in place: x[i] = sum of x[j], j < i, for i in [0, m]; one workgroup
__global__ __launch_bounds__(1024) void k_import_scan64(uint64_t* __restrict__ x, uint64_t m) {
    __shared__ uint64_t wsum[1024 / 64];
    uint64_t carry = 0;
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

__global__ __launch_bounds__(kImportThreads) void k_line_starts(ImportText t, const uint64_t* __restrict__ tile_base, uint64_t* __restrict__ line_start) {
    __shared__ uint32_t w_sum[kImportThreads / 64];
    const uint64_t at = ((uint64_t)blockIdx.x * kImportThreads + threadIdx.x) * kImportLaneBytes;
    uint32_t m = newline_mask(t, at);
    uint32_t all;
    uint64_t k = tile_base[blockIdx.x] + block_exclusive<uint32_t>((uint32_t)__popc(m), w_sum, &all) + 1u;      // (line 0 starts at byte 0)
    if (at == 0) line_start[0] = 0;
    for (; m; m &= m - 1u) line_start[k++] = at + (uint32_t)__builtin_ctz(m) + 1u;
}

// the bytes of line i without its '\n'
__device__ __forceinline__ uint64_t line_span(const ImportLines& l, uint64_t i, uint64_t* start) {
    const uint64_t a = l.line_start[i], e = i < l.n_newlines ? l.line_start[i + 1] - 1u : l.t.size;
    *start = a;
    return e - a;
}

__global__ __launch_bounds__(kImportThreads) void k_import_measure(ImportLines l, uint32_t* __restrict__ rec_len, uint64_t* __restrict__ group_sum,
                                                                  unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long w_sum[kImportThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kImportThreads + threadIdx.x;
    uint64_t length = 0;
    bool bad = false;
    if (i < l.n_lines) {
        uint64_t a;
        const uint64_t n = line_span(l, i, &a);
        bad = sampc::sam_record_length(l.t.text + a, n, l.refs, &length) != sampc::kParseOk;
        if (bad) length = 0;
        rec_len[i] = (uint32_t)length;                 // (a record is shorter than 2^31 bytes or bad)
    }
    const unsigned long long all = block_sum<unsigned long long>(length, w_sum);
    const unsigned long long mb = __ballot(bad);
    if (bad) atomicMin(acc + kImportAccFirstBad, (unsigned long long)(l.first_line + i));
    if (mb && (threadIdx.x & 63u) == 0) atomicAdd(acc + kImportAccBad, (unsigned long long)__popcll(mb));
    if (threadIdx.x == 0) group_sum[blockIdx.x] = all;
}

__global__ __launch_bounds__(kImportThreads) void k_import_offsets(const uint32_t* __restrict__ rec_len, const uint64_t* __restrict__ group_base,
                                                                  uint64_t n, uint64_t store_used, uint64_t* __restrict__ rec_off) {
    __shared__ uint64_t w_sum[kImportThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kImportThreads + threadIdx.x;
    uint64_t all;
    const uint64_t before = block_exclusive<uint64_t>(i < n ? rec_len[i] : 0u, w_sum, &all);
    if (i < n) rec_off[i] = store_used + group_base[blockIdx.x] + before;
}

__global__ __launch_bounds__(kImportThreads) void k_import_emit(ImportLines l, const uint32_t* __restrict__ rec_len, const uint64_t* __restrict__ rec_off,
                                                               uint8_t* __restrict__ store, unsigned long long* __restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * kImportThreads + threadIdx.x;
    bool wrong = false;
    if (i < l.n_lines && rec_len[i]) {
        uint64_t a;
        const uint64_t n = line_span(l, i, &a);
        wrong = sampc::sam_record_emit(l.t.text + a, n, l.refs, store + rec_off[i], rec_len[i]) != sampc::kParseOk;
    }
    const unsigned long long m = __ballot(wrong);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(acc + kImportAccOverrun, (unsigned long long)__popcll(m));
}

}  // namespace

void launch_import_count_newlines(const ImportText& t, uint64_t* d_tile_sum, hipStream_t stream) {
    if (!t.size) return;
    hipLaunchKernelGGL(k_count_newlines, dim3(import_text_tiles(t.size)), dim3(kImportThreads), 0, stream, t, d_tile_sum);
    SBX_HIP(hipGetLastError());
}

void launch_import_scan64(uint64_t* d_x, uint64_t m, hipStream_t stream) {
    hipLaunchKernelGGL(k_import_scan64, dim3(1), dim3(1024), 0, stream, d_x, m);
    SBX_HIP(hipGetLastError());
}

void launch_import_line_starts(const ImportText& t, const uint64_t* d_tile_base, uint64_t* d_line_start, hipStream_t stream) {
    if (!t.size) return;
    hipLaunchKernelGGL(k_line_starts, dim3(import_text_tiles(t.size)), dim3(kImportThreads), 0, stream, t, d_tile_base, d_line_start);
    SBX_HIP(hipGetLastError());
}

void launch_import_measure(const ImportLines& l, uint32_t* d_rec_len, uint64_t* d_group_sum, unsigned long long* d_acc, hipStream_t stream) {
    if (!l.n_lines) return;
    hipLaunchKernelGGL(k_import_measure, dim3(import_line_groups(l.n_lines)), dim3(kImportThreads), 0, stream, l, d_rec_len, d_group_sum, d_acc);
    SBX_HIP(hipGetLastError());
}

void launch_import_offsets(const uint32_t* d_rec_len, const uint64_t* d_group_base, uint64_t n, uint64_t store_used, uint64_t* d_rec_off,
                           hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_import_offsets, dim3(import_line_groups(n)), dim3(kImportThreads), 0, stream, d_rec_len, d_group_base, n, store_used, d_rec_off);
    SBX_HIP(hipGetLastError());
}

void launch_import_emit(const ImportLines& l, const uint32_t* d_rec_len, const uint64_t* d_rec_off, uint8_t* d_store, unsigned long long* d_acc,
                        hipStream_t stream) {
    if (!l.n_lines) return;
    hipLaunchKernelGGL(k_import_emit, dim3(import_line_groups(l.n_lines)), dim3(kImportThreads), 0, stream, l, d_rec_len, d_rec_off, d_store, d_acc);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
