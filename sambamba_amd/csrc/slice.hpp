// slice.hpp -- launchers of K18 (slice.hip): the edge logic of `sambamba slice` over the records K2 described in the edge runs.
#pragma once
#include "kernels.hpp"

namespace sbx {

// words of the accumulators K18a adds to
enum SliceAcc : uint32_t { kSliceAccEntries = 0, kSliceAccBytes = 1, kSliceAccBad = 2, kSliceAccWords = 3 };

struct SliceEdge { uint32_t ref_id, x; };                   // an edge position of a region (its beg or its end), sorted by (ref_id, x)
struct SliceBeg { uint32_t ref_id, beg, region, pad; };     // the start of region `region` (its place in the output), sorted by (ref_id, beg)

struct SliceSelectArgs {
    const uint8_t* U;               // inflated bytes of the edge runs (work-list coordinates)
    const RecDesc* desc;            // their records in file order, RecDesc::pad = the verdict of K2 (IndexArgs::filter_every)
    const int32_t* rec_ref;
    uint64_t n;                     // records
    uint64_t u_end;                 // no record ends behind this offset of U
    const SliceEdge* edges;
    uint32_t n_edges;
    const SliceBeg* begs;
    uint32_t n_begs;
    unsigned long long* edge_min;   // [n_edges] atomicMin: the lowest rec_off among the records whose last edge at or in front of them
                                    //           is this one (all ones: none); the suffix minimum over the edges of a contig is first_ge
    uint32_t* region_count;         // [n_begs] += R1 records of the region
    unsigned long long* region_bytes;   // [n_begs] += their bytes
    uint32_t* count;                // [n] out: R1 entries of the record (one per region whose R1 holds it)
    uint32_t* group_entries;        // [slice_groups(n)] out: entries per workgroup
    unsigned long long* acc;        // [kSliceAccWords]
};
constexpr uint32_t kSliceThreads = 256;
inline uint32_t slice_groups(uint64_t n) { return (uint32_t)((n + kSliceThreads - 1) / kSliceThreads); }
// K18a
void launch_slice_select(const SliceSelectArgs& a, hipStream_t stream);

struct SliceEmitArgs {
    SliceSelectArgs s;                  // as K18a saw it (count)
    const uint64_t* group_entry_base;   // exclusive scan of group_entries
    uint64_t* key;                      // [entries] out: 4 * region, in file order
    uint64_t* off;                      // [entries] out: rec_off
    uint32_t* len;                      // [entries] out: block_size + 4
};
// K18b
void launch_slice_emit(const SliceEmitArgs& a, hipStream_t stream);

}  // namespace sbx
