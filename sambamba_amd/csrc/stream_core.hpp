// stream_core.hpp -- the arithmetic of K21 (stream.hip) and of the streamed writer (engine_streamout.hpp): what one record of a
// batch puts into one staging window of the output stream.  `__host__ __device__`: K21 runs the very statements
// tests/native/stream_host.cpp checks on the CPU against a byte-wise restatement.
//
// The output stream is header + selected records in file order.  A record at [dest, dest + len) of the stream meets the window
// [w0, w1) in at most one stretch (sortc::clip_to_piece).  With a bin patch the record's bytes 14 and 15 are NOT part of any copy:
// the record is copied as two stretches, [0, 14) and [16, len), each clipped on its own, and the two bytes are written one by one,
// each only when its place in the stream lies inside the window -- so no byte of the window is written twice, whatever the clip.
// The patch is 16 bits at a byte offset the caller names: 14, the bin (fixbins), or 18, the flag (subsample); the same holds there.
#pragma once
#include "sort_core.hpp"

namespace sbx {
namespace streamc {

constexpr uint32_t kNoPatch = 0xFFFFFFFFu;      // PackArgs::bin of a record whose bin stays as it is
constexpr uint32_t kBinOffset = 14;             // the bin field: bytes 14 and 15 of a record, block_size field included
constexpr uint32_t kFlagOffset = 18;            // the flag field: bytes 18 and 19

struct PackPlan {
    uint32_t n_spans;               // 0 .. 2
    sortc::PieceClip span[2];       // span[k].len bytes from byte span[k].src of the record to byte span[k].dst of the window
    uint32_t n_bytes;               // 0 .. 2 single bytes of the patch
    uint64_t byte_dst[2];           // their places in the window
    uint8_t byte_val[2];
    SBX_SORT_HD uint64_t wrote() const {
        uint64_t w = n_bytes;
        for (uint32_t k = 0; k < n_spans; ++k) w += span[k].len;
        return w;
    }
};

// What the window [w0, w1) receives of a record of len bytes (>= patch_off + 2) that starts at byte dest of the stream; bin: kNoPatch,
// or the value bytes patch_off .. patch_off + 1 take (little endian).
SBX_SORT_HD void plan_record(uint64_t dest, uint64_t len, uint64_t w0, uint64_t w1, uint32_t bin, PackPlan* p, uint32_t patch_off = kBinOffset) {
    p->n_spans = 0;
    p->n_bytes = 0;
    if (bin == kNoPatch) {
        if (sortc::clip_to_piece(dest, dest + len, w0, w1, &p->span[0])) p->n_spans = 1;
        return;
    }
    sortc::PieceClip c;
    if (sortc::clip_to_piece(dest, dest + patch_off, w0, w1, &c)) p->span[p->n_spans++] = c;
    if (sortc::clip_to_piece(dest + patch_off + 2, dest + len, w0, w1, &c)) {
        c.src += patch_off + 2;
        p->span[p->n_spans++] = c;
    }
    for (uint32_t k = 0; k < 2; ++k) {
        const uint64_t at = dest + patch_off + k;
        if (at >= w0 && at < w1) {
            p->byte_dst[p->n_bytes] = at - w0;
            p->byte_val[p->n_bytes] = (uint8_t)(bin >> (8 * k));
            ++p->n_bytes;
        }
    }
}

// The record bytes that belong into the window [w0, w1) of a stream whose first hlen bytes are the header and that holds `end` bytes
// so far (end > w0): what K21's counter must show when the window is handed to the encoder.
SBX_SORT_HD uint64_t window_record_bytes(uint64_t w0, uint64_t w1, uint64_t hlen, uint64_t end) {
    const uint64_t hi = end < w1 ? end : w1;
    const uint64_t lo = hlen > w0 ? hlen : w0;
    return hi > lo ? hi - lo : 0;
}

}  // namespace streamc
}  // namespace sbx
