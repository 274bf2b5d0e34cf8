// bins.hpp -- launchers of K16 (bins.hip): the bin of every record against reg2bin of its position and CIGAR (bins_core.hpp).
#pragma once
#include "kernels.hpp"
#include "stream_core.hpp"

namespace sbx {

constexpr uint32_t kBinThreads = 256;
inline uint32_t bin_groups(uint64_t n) { return (uint32_t)((n + kBinThreads - 1) / kBinThreads); }

// K16a (`index -c`): words of its accumulator, kept over the batches of a pass
enum BinCheckAcc : uint32_t { kBinCheckBad = 0, kBinCheckFirst = 1, kBinCheckWords = 2 };
constexpr unsigned long long kBinCheckNone = ~0ull;         // what kBinCheckFirst starts with
// One lane per record of a batch (descriptors of an index-mode pass, record 0 of the batch being record rec_base of the file; the
// batch's inflated bytes end at u_end): a placed record (ref_id >= 0, pos >= 0) whose stored bin is not the expected one counts in
// acc[kBinCheckBad] and lowers acc[kBinCheckFirst] to its number in the file.  A record whose lengths contradict its block_size or
// the batch is not judged here.
void launch_check_bins(const uint8_t* d_U, const RecDesc* d_desc, const int32_t* d_rec_ref, uint64_t n, uint64_t rec_base, uint64_t u_end,
                       unsigned long long* d_acc, hipStream_t stream);

// K16b (`fixbins`): words of its accumulator
enum BinFixAcc : uint32_t { kBinFixBad = 0, kBinFixChanged = 1, kBinFixBytes = 2, kBinFixWords = 4 };
struct BinFixArgs {
    uint8_t* store;             // the resident record store; the batch has been copied into it
    const RecDesc* desc;        // the batch's descriptors: rec_off counts from the batch's U[0]
    uint64_t n;
    int64_t store_delta;        // store offset of a record = rec_off + store_delta
    uint64_t store_end;         // bytes of the store that are filled, this batch included
    uint64_t out_base;          // number of the batch's record 0 in the file
    uint64_t* off;              // out, [out_base + i]: offset of the record in the store
    uint32_t* len;              // out: its bytes, block_size field included (0 for a record that is refused)
    unsigned long long* acc;    // [kBinFixWords]
    uint32_t* bin_out;          // null: the resident path.  Otherwise the streamed path (engine_streamout.hpp): `store` is the batch's U
                                // (store_delta 0, store_end its end), nothing is stored into it, off / len are not written, and
                                // bin_out[i] = the expected bin of a record that carries another one, streamc::kNoPatch for every other
};
// One lane per record of a batch: bytes 14 .. 15 of the record in the store become the expected bin; records whose bin changes are
// counted, the bytes of all records added up, a record whose name and CIGAR run past its block_size is counted as bad and left alone.
void launch_fix_bins(const BinFixArgs& a, hipStream_t stream);

}  // namespace sbx
