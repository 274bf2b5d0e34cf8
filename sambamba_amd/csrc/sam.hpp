// sam.hpp -- launchers of K13 (sam.hip): the SAM text of the entries of `sambamba view`.
#pragma once
#include "kernels.hpp"
#include "sam_core.hpp"

namespace sbx {

// words of the accumulator of K13a / K13b
enum SamAcc : uint32_t { kSamAccBad = 0, kSamAccTooLong = 1, kSamAccOverrun = 2, kSamAccWords = 4 };

// entry i is record perm[i]: len[perm[i]] bytes at store + off[perm[i]]
struct SamEntries {
    const uint8_t* store;
    const uint64_t* off;
    const uint32_t* len;
    const uint32_t* perm;
    uint64_t n;
    samc::RefNames refs;            // device pointers
};

// K13a: line_len[i] = bytes of the line of entry i (0 for a malformed record, counted in acc[kSamAccBad]; a line of 2^32 bytes or more
// counts in acc[kSamAccTooLong]); group_sum[g] = the bytes of workgroup g -- kGroupThreads entries, group_count(n) words: launch_scan64
// and launch_group_offsets (scan.hpp) turn them into line_off[0, n], the offset of every line and in line_off[n] all bytes.
void launch_sam_measure(const SamEntries& e, uint32_t* d_line_len, uint64_t* d_group_sum, unsigned long long* d_acc, hipStream_t stream);
// The pieces of the text: piece k holds the lines [first[k], first[k + 1]), as many consecutive lines as fit `budget` bytes and at
// least one.  d_first == nullptr: only *d_n_pieces is written; otherwise d_first[0 .. *d_n_pieces] (the last word = n) and the
// offsets of those lines, d_first_off[0 .. *d_n_pieces], too.
void launch_sam_pieces(const uint64_t* d_line_off, uint64_t n, uint64_t budget, uint32_t* d_first, uint64_t* d_first_off, uint32_t* d_n_pieces,
                       hipStream_t stream);
// K13b: the lines of entries [i0, i1) into piece + (line_off[i] - line_off[i0]); a line whose emission disagrees with its measured
// length counts in acc[kSamAccOverrun] (and writes nothing outside its own bytes).
void launch_sam_emit(const SamEntries& e, const uint32_t* d_line_len, const uint64_t* d_line_off, uint64_t i0, uint64_t i1, uint8_t* d_piece,
                     unsigned long long* d_acc, hipStream_t stream);

}  // namespace sbx
