// samparse.hpp -- launchers of K15 (samparse.hip): the lines of a chunk of SAM text turned into BAM records in the resident store.
#pragma once
#include "kernels.hpp"
#include "samparse_core.hpp"

namespace sbx {

// words of the accumulator of K15b / K15c
enum ImportAcc : uint32_t { kImportAccBad = 0, kImportAccFirstBad = 1, kImportAccOverrun = 2, kImportAccWords = 4 };
constexpr unsigned long long kImportNoBadLine = ~0ull;      // what kImportAccFirstBad starts with

constexpr uint32_t kImportThreads = 256;
constexpr uint32_t kImportLaneBytes = 16;                   // text bytes one lane of K15a looks at: one 16-byte load
constexpr uint32_t kImportTileBytes = kImportThreads * kImportLaneBytes;
inline uint32_t import_text_tiles(uint64_t size) { return (uint32_t)((size + kImportTileBytes - 1) / kImportTileBytes); }
inline uint32_t import_line_groups(uint64_t n) { return (uint32_t)((n + kImportThreads - 1) / kImportThreads); }

// a chunk of text on the device: `size` bytes at a 16-byte boundary, readable up to the next multiple of 16
struct ImportText {
    const uint8_t* text;
    uint64_t size;
};

// K15a, first half: tile_sum[t] = the '\n' bytes of text tile t (import_text_tiles(size) words); import_scan64 over them gives the
// number of the first line that starts behind tile t, and in its last word the '\n' bytes of the chunk.
void launch_import_count_newlines(const ImportText& t, uint64_t* d_tile_sum, hipStream_t stream);
// in place, one workgroup: x[i] = sum of x[j], j < i, for i in [0, m]
void launch_import_scan64(uint64_t* d_x, uint64_t m, hipStream_t stream);
// K15a, second half: line_start[0] = 0 and line_start[k] = the byte behind the k-th '\n' (n_newlines + 1 words)
void launch_import_line_starts(const ImportText& t, const uint64_t* d_tile_base, uint64_t* d_line_start, hipStream_t stream);

// the lines of a chunk: line i is text[line_start[i], line_start[i + 1] - 1) for i < n_newlines, the last line of a text that does not
// end in '\n' is text[line_start[n_newlines], size)
struct ImportLines {
    ImportText t;
    const uint64_t* line_start;
    uint64_t n_newlines, n_lines;       // n_lines = n_newlines, + 1 when the text does not end in '\n'
    uint64_t first_line;                // 1-based number of line 0 in the file
    sampc::RefTable refs;               // device pointers
};
// K15b: rec_len[i] = bytes of the record of line i (0 for a line outside the grammar: counted in acc[kImportAccBad], its number
// lowers acc[kImportAccFirstBad]); group_sum[g] = the record bytes of lines [256 g, 256 g + 256).
void launch_import_measure(const ImportLines& l, uint32_t* d_rec_len, uint64_t* d_group_sum, unsigned long long* d_acc, hipStream_t stream);
// rec_off[i] = store_used + group_base[i / 256] + the lengths in front of i inside its group
void launch_import_offsets(const uint32_t* d_rec_len, const uint64_t* d_group_base, uint64_t n, uint64_t store_used, uint64_t* d_rec_off,
                           hipStream_t stream);
// K15c: the record of line i at store + rec_off[i], rec_len[i] bytes; a record whose emission disagrees with its measured length
// counts in acc[kImportAccOverrun] (and writes nothing outside its own bytes).
void launch_import_emit(const ImportLines& l, const uint32_t* d_rec_len, const uint64_t* d_rec_off, uint8_t* d_store, unsigned long long* d_acc,
                        hipStream_t stream);

}  // namespace sbx
