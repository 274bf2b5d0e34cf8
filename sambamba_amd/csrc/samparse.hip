// samparse.hip -- K15: the lines of a chunk of SAM text (`sambamba view -S -f bam`, parseAlignmentLine of BioD's sam_alignment.rl)
// turned into BAM records in the resident record store.
//
//   K15a (lines.hip)       the line starts of the chunk.
//   K15b k_import_measure  one lane per line: the line walker of samparse_core.hpp with the sink that only adds lengths up.  The
//                          record's length is stored, the lengths of a workgroup are summed, lines outside the grammar are counted
//                          once per wave and the lowest line number among them is kept (atomicMin).  launch_scan64 over the sums and
//                          launch_group_offsets (scan.hip) give every record its 64-bit offset behind the fill of the store.
//   K15c k_import_emit     one lane per line: the walker again, with the sink that writes (fmt::RowSink: eight bytes per store,
//                          every store inside the lane's own record).
//   K15d k_import_emit_window  the streamed path (engine_import.cpp): no store; the records of the chunk are a stretch of the output
//                          stream and one launch fills one staging window of it.  One lane per line as K15c; a lane whose record has
//                          no byte in the window does nothing, one whose record lies inside runs K15c's statements, one whose record
//                          straddles an edge runs the walker with sampc::WindowSink.  The bytes written are summed per workgroup
//                          into the writer's counter (as K21's).
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

// the bytes of line i without its '\n'
__device__ __forceinline__ uint64_t line_span(const ImportLines& l, uint64_t i, uint64_t* start) {
    const uint64_t a = l.line_start[i], e = i < l.n_newlines ? l.line_start[i + 1] - 1u : l.t.size;
    *start = a;
    return e - a;
}

__global__ __launch_bounds__(kGroupThreads) void k_import_measure(ImportLines l, uint32_t* __restrict__ rec_len, uint64_t* __restrict__ group_sum,
                                                                  unsigned long long* __restrict__ acc) {
    __shared__ unsigned long long w_sum[kGroupThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
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

__global__ __launch_bounds__(kGroupThreads) void k_import_emit(ImportLines l, const uint32_t* __restrict__ rec_len, const uint64_t* __restrict__ rec_off,
                                                               uint8_t* __restrict__ store, unsigned long long* __restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    bool wrong = false;
    if (i < l.n_lines && rec_len[i]) {
        uint64_t a;
        const uint64_t n = line_span(l, i, &a);
        wrong = sampc::sam_record_emit(l.t.text + a, n, l.refs, store + rec_off[i], rec_len[i]) != sampc::kParseOk;
    }
    const unsigned long long m = __ballot(wrong);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(acc + kImportAccOverrun, (unsigned long long)__popcll(m));
}

// K15d: the records of the chunk as a part of the output stream (rec_off counts from the stream's first byte), of which the staging
// window [w0, w1) is filled: stream byte p at window[p - w0].  A record wholly inside is K15c's; one that straddles an edge -- at
// most two of a launch, or one that covers the window -- goes through the clipping sink.
__global__ __launch_bounds__(kGroupThreads) void k_import_emit_window(ImportLines l, const uint32_t* __restrict__ rec_len,
                                                                      const uint64_t* __restrict__ rec_off, uint8_t* __restrict__ window, uint64_t w0,
                                                                      uint64_t w1, unsigned long long* __restrict__ acc,
                                                                      unsigned long long* __restrict__ wrote_acc) {
    __shared__ unsigned long long w_sum[kGroupThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    bool wrong = false;
    uint64_t wrote = 0;
    if (i < l.n_lines && rec_len[i]) {
        const uint64_t off = rec_off[i], len = rec_len[i];
        if (off < w1 && off + len > w0) {
            uint64_t a;
            const uint64_t n = line_span(l, i, &a);
            if (off >= w0 && off + len <= w1) {
                wrong = sampc::sam_record_emit(l.t.text + a, n, l.refs, window + (off - w0), len) != sampc::kParseOk;
                wrote = len;
            } else {
                wrong = sampc::sam_record_emit_window(l.t.text + a, n, l.refs, off, len, window, w0, w1, &wrote) != sampc::kParseOk;
            }
        }
    }
    const unsigned long long all = block_sum<unsigned long long>(wrote, w_sum);
    if (all && threadIdx.x == 0) atomicAdd(wrote_acc, all);
    const unsigned long long m = __ballot(wrong);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(acc + kImportAccOverrun, (unsigned long long)__popcll(m));
}

}  // namespace

void launch_import_emit_window(const ImportLines& l, const uint32_t* d_rec_len, const uint64_t* d_rec_off, uint8_t* d_window, uint64_t w0, uint64_t w1,
                               unsigned long long* d_acc, unsigned long long* d_wrote, hipStream_t stream) {
    if (!l.n_lines) return;
    hipLaunchKernelGGL(k_import_emit_window, dim3(group_count(l.n_lines)), dim3(kGroupThreads), 0, stream, l, d_rec_len, d_rec_off, d_window, w0, w1,
                       d_acc, d_wrote);
    SBX_HIP(hipGetLastError());
}

void launch_import_measure(const ImportLines& l, uint32_t* d_rec_len, uint64_t* d_group_sum, unsigned long long* d_acc, hipStream_t stream) {
    if (!l.n_lines) return;
    hipLaunchKernelGGL(k_import_measure, dim3(group_count(l.n_lines)), dim3(kGroupThreads), 0, stream, l, d_rec_len, d_group_sum, d_acc);
    SBX_HIP(hipGetLastError());
}

void launch_import_emit(const ImportLines& l, const uint32_t* d_rec_len, const uint64_t* d_rec_off, uint8_t* d_store, unsigned long long* d_acc,
                        hipStream_t stream) {
    if (!l.n_lines) return;
    hipLaunchKernelGGL(k_import_emit, dim3(group_count(l.n_lines)), dim3(kGroupThreads), 0, stream, l, d_rec_len, d_rec_off, d_store, d_acc);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
