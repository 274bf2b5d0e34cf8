// fasta.hpp -- launchers of K17 (fasta.hip): the inner lines of a chunk of FASTA text (fasta_core.hpp) reduced to one FastaSeg per
// header line among them.  The line starts are K15a's (lines.hpp).
#pragma once
#include "fasta_core.hpp"
#include "lines.hpp"

namespace sbx {

// words of K17's accumulator (per chunk)
enum FastaAcc : uint32_t { kFastaAccBare = 0, kFastaAccFirstBare = 1, kFastaAccWords = 2 };

// the inner lines of a chunk: inner line k (1 <= k < n_newlines) is text[line_start[k], line_start[k + 1] - 1)
struct FastaLines {
    TextChunk t;
    const uint64_t* line_start;         // K15a: n_newlines + 1 words
    uint64_t n_newlines;
    uint32_t crlf;
};
inline uint64_t fasta_inner_lines(uint64_t n_newlines) { return n_newlines >= 2 ? n_newlines - 1 : 0; }

// K17a: group_sum[g] = the header lines among inner lines [256 g + 1, 256 g + 257); launch_scan64 over the groups numbers the segments
void launch_fasta_count_headers(const FastaLines& l, uint64_t* d_group_sum, hipStream_t stream);
// K17b: seg[0 .. n_headers] (set up by the caller: seq_bytes 0, first_line kNoLine) receive the sums, minima and header lines;
// acc[kFastaAccBare] += the inner lines that end in a bare '\n' ("\r\n" mode), acc[kFastaAccFirstBare] = min of their numbers k
void launch_fasta_segments(const FastaLines& l, const uint64_t* d_group_base, fastac::FastaSeg* d_seg, unsigned long long* d_acc, hipStream_t stream);
// seg[0 .. n): {0, kNoLine, 0, 0}
void launch_fasta_clear_segments(fastac::FastaSeg* d_seg, uint64_t n, hipStream_t stream);

}  // namespace sbx
