// lines.hpp -- launchers of K15a (lines.hip): where the lines of a chunk of text start.  The first step of K15 (samparse.hip) and of K17
// (fasta.hip).
#pragma once
#include "kernels.hpp"

namespace sbx {

constexpr uint32_t kLineLaneBytes = 16;                     // text bytes one lane of K15a looks at: one 16-byte load
constexpr uint32_t kTextTileBytes = kGroupThreads * kLineLaneBytes;
inline uint32_t text_tiles(uint64_t size) { return (uint32_t)((size + kTextTileBytes - 1) / kTextTileBytes); }

// a chunk of text on the device: `size` bytes at a 16-byte boundary, readable up to the next multiple of 16
struct TextChunk {
    const uint8_t* text;
    uint64_t size;
};

// K15a, first half: tile_sum[t] = the '\n' bytes of text tile t (text_tiles(size) words); launch_scan64 over them gives the number of
// the first line that starts behind tile t, and in its last word the '\n' bytes of the chunk.
void launch_count_newlines(const TextChunk& t, uint64_t* d_tile_sum, hipStream_t stream);
// K15a, second half: line_start[0] = 0 and line_start[k] = the byte behind the k-th '\n' (n_newlines + 1 words)
void launch_line_starts(const TextChunk& t, const uint64_t* d_tile_base, uint64_t* d_line_start, hipStream_t stream);

}  // namespace sbx
