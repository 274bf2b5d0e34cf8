// samparse.hpp -- launchers of K15 (samparse.hip): the lines of a chunk of SAM text turned into BAM records in the resident store.
#pragma once
#include "lines.hpp"
#include "samparse_core.hpp"

namespace sbx {

// words of the accumulator of K15b / K15c
enum ImportAcc : uint32_t { kImportAccBad = 0, kImportAccFirstBad = 1, kImportAccOverrun = 2, kImportAccWords = 4 };
constexpr unsigned long long kImportNoBadLine = ~0ull;      // what kImportAccFirstBad starts with

// the lines of a chunk: line i is text[line_start[i], line_start[i + 1] - 1) for i < n_newlines, the last line of a text that does not
// end in '\n' is text[line_start[n_newlines], size)
struct ImportLines {
    TextChunk t;
    const uint64_t* line_start;         // K15a (lines.hpp)
    uint64_t n_newlines, n_lines;       // n_lines = n_newlines, + 1 when the text does not end in '\n'
    uint64_t first_line;                // 1-based number of line 0 in the file
    sampc::RefTable refs;               // device pointers
};
// K15b: rec_len[i] = bytes of the record of line i (0 for a line outside the grammar: counted in acc[kImportAccBad], its number
// lowers acc[kImportAccFirstBad]); group_sum[g] = the record bytes of lines [256 g, 256 g + 256) -- kGroupThreads lines, group_count(n_lines)
// words: launch_scan64 and launch_group_offsets (scan.hpp) turn them into the store offset of every record.
void launch_import_measure(const ImportLines& l, uint32_t* d_rec_len, uint64_t* d_group_sum, unsigned long long* d_acc, hipStream_t stream);
// K15c: the record of line i at store + rec_off[i], rec_len[i] bytes; a record whose emission disagrees with its measured length
// counts in acc[kImportAccOverrun] (and writes nothing outside its own bytes).
void launch_import_emit(const ImportLines& l, const uint32_t* d_rec_len, const uint64_t* d_rec_off, uint8_t* d_store, unsigned long long* d_acc,
                        hipStream_t stream);
// K15d: rec_off[i] is the place of record i in the output stream; the bytes of the records that lie in [w0, w1) of the stream are
// written at d_window + (place - w0) and nothing else is (d_window holds w1 - w0 bytes).  *d_wrote grows by the number of bytes
// written; a record whose emission disagrees with its measured length counts in acc[kImportAccOverrun].
void launch_import_emit_window(const ImportLines& l, const uint32_t* d_rec_len, const uint64_t* d_rec_off, uint8_t* d_window, uint64_t w0, uint64_t w1,
                               unsigned long long* d_acc, unsigned long long* d_wrote, hipStream_t stream);

}  // namespace sbx
