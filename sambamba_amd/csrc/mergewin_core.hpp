// mergewin_core.hpp -- the pieces of a REWRITTEN record, clipped to a window of the merged stream: what K11c (k_merge_window_scatter,
// merge.hip) writes of one record of a replayed batch when sbx_merge_bam has no record store (engine_merge.cpp, the windowed path).
//
// K11b (k_merge_rewrite) writes a record in up to six stretches: the 36 fixed bytes with block_size, ref_id and next_ref_id
// replaced; the source bytes up to the first patch; the new id of that patch; the source bytes up to the second patch; its new id;
// the tail.  A patch replaces old_len bytes at offset `at` of the record as it is in its input by new_len bytes of the rename
// table's blob; patches are ascending, lie behind the fixed part and do not overlap (K11a leaves them so in MergeBatch).  Here
// the same walk is done for a record that starts at `dest` of the merged stream, and every stretch is clipped ON ITS OWN to the
// window [w0, w1) with sortc::clip_to_piece: a window edge may fall inside a replaced word, inside a new id or exactly between a
// patch and the stretch behind it, and no byte of the window is written twice or left out, because the stretches tile
// [dest, dest + new_len) and the clip of each is exact.
//
// `__host__ __device__`, no HIP included: the kernel runs the very statements tests/native/mergewin_host.cpp checks.
#pragma once
#include "sort_core.hpp"

namespace sbx {
namespace mergewin {

constexpr uint32_t kFixedBytes = 36;      // block_size + the 32 fixed bytes: what K11b writes byte by byte
constexpr uint32_t kMaxPatches = 2;
constexpr uint32_t kMaxStretches = 7;     // room in a plan; two patches make six

enum StretchKind : uint32_t {
    kStretchFixed = 0,      // src: the first of the 36 fixed bytes of the rewritten record to write
    kStretchSource = 1,     // src: offset in the record as it is in its input
    kStretchBlob = 2,       // src: offset in the rename table's blob
};

// one replaced id: old_len bytes at `at` of the input's record become the new_len bytes at new_off of the blob
struct Patch { uint32_t at, old_len, new_len, new_off; };

// `len` (> 0) bytes of `kind` from `src` to byte `dst` of the window
struct Stretch { uint32_t kind; uint64_t src, dst, len; };

// Calls emit(kind, src, dst, len) for every stretch of the rewritten record that has a byte in [w0, w1), in stream order.
// old_len / new_len: block_size + 4 of the record as read and as written; new_len == old_len + the sum of (new_len - old_len) over
// the np patches (the caller's to guarantee: K11a computes new_len so).
template <class Emit>
SBX_SORT_HD void for_each_stretch(uint32_t old_len, uint32_t new_len, const Patch* patch, uint32_t np, uint64_t dest, uint64_t w0,
                                  uint64_t w1, Emit&& emit) {
    (void)new_len;
    sortc::PieceClip c;
    if (sortc::clip_to_piece(dest, dest + kFixedBytes, w0, w1, &c)) emit((uint32_t)kStretchFixed, c.src, c.dst, c.len);
    uint64_t s_pos = kFixedBytes, d_pos = dest + kFixedBytes;
    for (uint32_t k = 0; k < kMaxPatches && k < np; ++k) {
        const Patch p = patch[k];
        const uint64_t gap = (uint64_t)p.at - s_pos;
        if (sortc::clip_to_piece(d_pos, d_pos + gap, w0, w1, &c)) emit((uint32_t)kStretchSource, s_pos + c.src, c.dst, c.len);
        d_pos += gap;
        if (sortc::clip_to_piece(d_pos, d_pos + p.new_len, w0, w1, &c)) emit((uint32_t)kStretchBlob, (uint64_t)p.new_off + c.src, c.dst, c.len);
        d_pos += p.new_len;
        s_pos = (uint64_t)p.at + p.old_len;
    }
    if (sortc::clip_to_piece(d_pos, d_pos + ((uint64_t)old_len - s_pos), w0, w1, &c)) emit((uint32_t)kStretchSource, s_pos + c.src, c.dst, c.len);
}

// the same as a list: out has room for kMaxStretches; returns how many were written
SBX_SORT_HD uint32_t plan_record_window(uint32_t old_len, uint32_t new_len, const Patch* patch, uint32_t np, uint64_t dest, uint64_t w0,
                                        uint64_t w1, Stretch* out) {
    uint32_t n = 0;
    for_each_stretch(old_len, new_len, patch, np, dest, w0, w1, [&](uint32_t kind, uint64_t src, uint64_t dst, uint64_t len) {
        out[n].kind = kind; out[n].src = src; out[n].dst = dst; out[n].len = len;
        ++n;
    });
    return n;
}

// byte b (0 .. 35) of the fixed part of the rewritten record: the word it lies in is the new block_size (word 0), the new ref_id
// (word 1), the new next_ref_id (word 6) or the input's word -- K11b's statement
SBX_SORT_HD uint8_t fixed_byte(uint32_t b, uint32_t new_block_size, uint32_t new_ref, uint32_t new_next, uint32_t source_word) {
    const uint32_t w = b >> 2;
    const uint32_t v = w == 0 ? new_block_size : w == 1 ? new_ref : w == 6 ? new_next : source_word;
    return (uint8_t)(v >> (8 * (b & 3u)));
}

}  // namespace mergewin
}  // namespace sbx
