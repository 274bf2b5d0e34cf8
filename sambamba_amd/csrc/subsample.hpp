// subsample.hpp -- launchers of K22 (subsample.hip): per-position coverage of a whole file and the verdict of `subsample` per record.
#pragma once
#include "kernels.hpp"
#include "stream_core.hpp"
#include "subsample_core.hpp"

namespace sbx {

constexpr uint32_t kCovThreads = 256;
inline uint32_t cov_groups(uint64_t n) { return (uint32_t)((n + kCovThreads - 1) / kCovThreads); }
constexpr uint64_t kMaxCovTiles = (1ull << 24) - 1;     // tiles of D the scan takes (launch_cov_scan)

// words of the accumulator K22a and K22c share, kept over the batches of both passes
enum CovAcc : uint32_t {
    kCovBad = 0,            // K22a, K22c: records whose name and CIGAR run past their block_size or the batch
    kCovCounted = 1,        // K22a: counted records
    kCovOver = 2,           // K22c: counted records with cov > max_cov
    kCovDropped = 3,        // K22c: ... that the hash drops
    kCovBytes = 4,          // K22c: block_size + 4 of the records the writer receives
    kCovMaxSeen = 5,        // K22c: the largest cov of a counted record (atomicMax)
    kCovWords = 8
};

struct CovArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records
    uint64_t n;
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    const uint64_t* base;           // [n_ref + 1] subc::slot_bases on the device
    int32_t n_ref;
    uint32_t* D;                    // the coverage array: base[n_ref] slots, rounded up to whole tiles of subc::kCovTile words
    unsigned long long* acc;        // [kCovWords]
    // K22c only
    uint32_t max_cov;
    uint32_t* count;                // [n] with -r: 1 for a record that is written, 0 for a dropped one (PackArgs::count); else null
    uint32_t* patch;                // [n] without -r: streamc::kNoPatch, or flag | 0x200 of a dropped record (PackArgs::bin at byte 18)
};
// K22a: every counted record of the batch adds +1 at the slot of its pos and -1 at the slot of its e
void launch_cov_mark(const CovArgs& a, hipStream_t stream);
// K22b: D[i] = sum of D[j], j <= i, over n_tiles * subc::kCovTile words, in place; tile_sum: n_tiles + 2 words of scratch
void launch_cov_scan(uint32_t* D, uint64_t n_tiles, uint64_t* tile_sum, hipStream_t stream);
// K22c: the verdict of every record of the batch from the scanned D, into count or patch
void launch_cov_verdict(const CovArgs& a, hipStream_t stream);

}  // namespace sbx
