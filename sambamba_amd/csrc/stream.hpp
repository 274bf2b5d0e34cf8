// stream.hpp -- launchers of K21 (stream.hip): the selected records of one described batch, in file order, into a staging window of
// the output stream (engine_streamout.hpp).
#pragma once
#include "kernels.hpp"
#include "scan.hpp"
#include "stream_core.hpp"

namespace sbx {

constexpr uint32_t kPackThreads = 256;
inline uint32_t pack_groups(uint64_t n) { return (uint32_t)((n + kPackThreads - 1) / kPackThreads); }

struct PackArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records
    uint64_t n;                     // records of the batch
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    const uint32_t* count;          // [n] K12a's verdict (ViewSelectArgs::count; 0: not selected); null: every record is selected
    const uint32_t* bin;            // [n] streamc::kNoPatch or the value of the record's 16-bit field at patch_off; null: no record is patched
    uint32_t patch_off = streamc::kBinOffset;      // byte offset of that field in the record: the bin (14), or streamc::kFlagOffset
    uint64_t stream_base;           // where the batch's first selected record starts in the output stream
    uint64_t* group_sum;            // [pack_groups(n) + 1] scratch of launch_pack_offsets
    uint64_t* dest;                 // [n + 1] launch_pack_offsets -> launch_pack_records: start of the record in the output stream
    uint32_t* len;                  // [n]                                            its bytes; 0: the record takes no part
    uint64_t w0, w1;                // the window: bytes [w0, w1) of the stream
    uint8_t* window;                // w1 - w0 bytes
    unsigned long long* acc;        // [1] += the bytes launch_pack_records wrote
};
// Once per batch: len[i] (block_size + 4 of a selected record whose frame lies inside the batch, else 0) and dest[i] = stream_base +
// the lengths of the records in front of i (dest[n]: behind the batch's last record).
void launch_pack_offsets(const PackArgs& a, hipStream_t stream);
// Once per (batch, window): the bytes of the batch's records that lie in [w0, w1), from U to window + (dest - w0).
void launch_pack_records(const PackArgs& a, hipStream_t stream);

}  // namespace sbx
