// fasta.hip -- K17: the inner lines of a chunk of FASTA text (`sambamba index -F`, buildFai of BioD's bio/std/file/fai.d) reduced to
// one FastaSeg per header line among them.  What a line is and what a segment holds: fasta_core.hpp.
//
//   K15a (lines.hip)          the '\n' bytes of the chunk counted per 4 KiB tile in 16-byte loads, scanned, and the line starts stored.
//   K17a k_fasta_count_headers one lane per inner line: is its first byte '>'; block_sum per 256 lines; launch_scan64 over the groups.
//   K17b k_fasta_segments     the same lanes: segment number = scanned base of the group + block_exclusive of the header flags (+ 1 on
//                             a header); a header lane stores its line's offset and length; the sequence lanes add their lengths up
//                             and take the minimum of (line number << 32 | length) over the lines that are not empty -- the first
//                             such line, whose length is the record's line length.  Lines of one segment are neighbours, so a
//                             workgroup whose first and last line share a segment reduces through LDS and issues one atomicAdd and
//                             one atomicMin; a workgroup with a header inside does the same per wave, and a wave with a header inside
//                             per lane.  Lines that end in a bare '\n' in "\r\n" mode are counted once per wave.
//
// The bound this sits under: the text is read twice in 16-byte loads that coalesce (K15a), then one byte at each end of
// every line twice (K17a, K17b: two scattered bytes per ~61 bytes of a wrapped file) next to 8 bytes of line start per line written
// once and read three times.  What leaves the device is 32 bytes per header line.  NOTHING here has a measured time.
#include "common.hpp"
#include "fasta.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

using fastac::FastaSeg;

__global__ __launch_bounds__(kGroupThreads) void k_fasta_clear_segments(FastaSeg* __restrict__ seg, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    if (i < n) seg[i] = FastaSeg{0, fastac::kNoLine, 0, 0};
}

__global__ __launch_bounds__(kGroupThreads) void k_fasta_count_headers(FastaLines l, uint64_t* __restrict__ group_sum) {
    __shared__ uint32_t w_sum[kGroupThreads / 64];
    const uint64_t j = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x;
    // (inner line j + 1 starts behind a '\n' and ends at a later one: its first byte lies inside the chunk)
    const bool header = j + 1 < l.n_newlines && l.t.text[l.line_start[j + 1]] == '>';
    const uint32_t all = block_sum<uint32_t>(header ? 1u : 0u, w_sum);
    if (threadIdx.x == 0) group_sum[blockIdx.x] = all;
}

__global__ __launch_bounds__(kGroupThreads) void k_fasta_segments(FastaLines l, const uint64_t* __restrict__ group_base, FastaSeg* __restrict__ seg,
                                                                  unsigned long long* __restrict__ acc) {
    constexpr uint32_t kWaves = kGroupThreads / 64;
    __shared__ uint32_t w_cnt[kWaves];
    __shared__ unsigned long long w_sum[kWaves], w_min[kWaves];
    __shared__ uint64_t s_ends[2];
    const uint64_t j = (uint64_t)blockIdx.x * kGroupThreads + threadIdx.x, k = j + 1;
    const bool live = k < l.n_newlines;
    fastac::InnerLine line{0, false, false};
    uint64_t a = 0;
    if (live) {
        a = l.line_start[k];
        line = fastac::inner_line(l.t.text, a, l.line_start[k + 1] - 1u, l.crlf != 0);
    }
    const bool header = live && line.header;
    uint32_t n_headers;
    const uint64_t s = group_base[blockIdx.x] + block_exclusive<uint32_t>(header ? 1u : 0u, w_cnt, &n_headers) + (header ? 1u : 0u);
    const bool bare = live && line.bare;
    const unsigned long long mb = __ballot(bare);
    if (bare) atomicMin(acc + kFastaAccFirstBare, (unsigned long long)k);
    if (mb && (threadIdx.x & 63u) == 0) atomicAdd(acc + kFastaAccBare, (unsigned long long)__popcll(mb));
    if (header) { seg[s].hdr_off = a; seg[s].hdr_len = line.len; }
    const bool sequence = live && !header;
    const unsigned long long len = sequence ? line.len : 0ull;
    const unsigned long long key = sequence ? fastac::first_line_key(k, line.len) : fastac::kNoLine;
    if (threadIdx.x == 0) s_ends[0] = s;                                                    // (thread 0 of a launched workgroup is live)
    if (live && (k + 1 == l.n_newlines || threadIdx.x == kGroupThreads - 1)) s_ends[1] = s;
    __syncthreads();
    if (s_ends[0] == s_ends[1]) {                       // one segment for the whole workgroup
        const unsigned long long sum = block_sum<unsigned long long>(len, w_sum);
        const unsigned long long wm = wave_min<unsigned long long>(key);
        if ((threadIdx.x & 63u) == 0) w_min[threadIdx.x >> 6] = wm;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long m = w_min[0];
            for (uint32_t w = 1; w < kWaves; ++w) m = w_min[w] < m ? w_min[w] : m;
            if (sum) atomicAdd((unsigned long long*)&seg[s].seq_bytes, sum);
            if (m != fastac::kNoLine) atomicMin((unsigned long long*)&seg[s].first_line, m);
        }
        return;
    }
    if (!__ballot(live)) return;
    const uint64_t s0 = __shfl((unsigned long long)s, 0, 64);                                // (lanes are in line order: lane 0 is live)
    if (!__ballot(live && s != s0)) {                   // one segment for the wave
        const unsigned long long sum = wave_sum<unsigned long long>(len), m = wave_min<unsigned long long>(key);
        if ((threadIdx.x & 63u) == 0) {
            if (sum) atomicAdd((unsigned long long*)&seg[s0].seq_bytes, sum);
            if (m != fastac::kNoLine) atomicMin((unsigned long long*)&seg[s0].first_line, m);
        }
        return;
    }
    if (sequence && len) {
        atomicAdd((unsigned long long*)&seg[s].seq_bytes, len);
        atomicMin((unsigned long long*)&seg[s].first_line, key);
    }
}

}  // namespace

void launch_fasta_clear_segments(fastac::FastaSeg* d_seg, uint64_t n, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_fasta_clear_segments, dim3(group_count(n)), dim3(kGroupThreads), 0, stream, d_seg, n);
    SBX_HIP(hipGetLastError());
}

void launch_fasta_count_headers(const FastaLines& l, uint64_t* d_group_sum, hipStream_t stream) {
    const uint64_t n = fasta_inner_lines(l.n_newlines);
    if (!n) return;
    hipLaunchKernelGGL(k_fasta_count_headers, dim3(group_count(n)), dim3(kGroupThreads), 0, stream, l, d_group_sum);
    SBX_HIP(hipGetLastError());
}

void launch_fasta_segments(const FastaLines& l, const uint64_t* d_group_base, fastac::FastaSeg* d_seg, unsigned long long* d_acc, hipStream_t stream) {
    const uint64_t n = fasta_inner_lines(l.n_newlines);
    if (!n) return;
    hipLaunchKernelGGL(k_fasta_segments, dim3(group_count(n)), dim3(kGroupThreads), 0, stream, l, d_group_base, d_seg, d_acc);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
