// view.hpp -- launchers of K12 (view.hip): the record selection of `sambamba view`.
#pragma once
#include "kernels.hpp"

namespace sbx {

// words of the accumulators K12a adds to over the batches of a file
enum ViewAcc : uint32_t { kViewAccEntries = 0, kViewAccRecords = 1, kViewAccBytes = 2, kViewAccBad = 3, kViewAccWords = 4 };

struct ViewSelectArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records, RecDesc::pad = the verdict of K2 (IndexArgs::filter_every)
    const int32_t* rec_ref;
    uint64_t n;                     // records of the batch
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    uint32_t flags_set, flags_unset;    // --num-filter (0 / 0: every record)
    uint32_t subsample;             // != 0: -s
    uint64_t seed, threshold;
    const sbx_region* regions;      // device copy; ref_id 0xFFFFFFFF = "*"
    uint32_t n_regions;             // 0: no region part
    uint32_t regions_merged;        // != 0: disjoint and sorted by (ref_id, start) -- a record counts once (binary search);
                                    // 0: the listed regions, a record counts once per region it overlaps
    uint32_t with_lengths;          // != 0: a selected record's block_size is read and checked (BAM output)
    uint32_t* count;                // [n] out: entries of the record; null for -c
    uint32_t* group_entries;        // [view_groups(n)] out: entries per workgroup; null for -c
    uint32_t* group_records;        // [view_groups(n)] out: selected records per workgroup; null for -c
    unsigned long long* acc;        // [kViewAccWords]
    const uint16_t* invalid;        // [n] the masks of K19 (valid.hip), or null: a record whose mask is not 0 is not selected and is not
                                    // counted as malformed either, whatever RecDesc::pad says (view -v)
};
constexpr uint32_t kViewThreads = 256;
inline uint32_t view_groups(uint64_t n) { return (uint32_t)((n + kViewThreads - 1) / kViewThreads); }
// K12a
void launch_view_select(const ViewSelectArgs& a, hipStream_t stream);

struct ViewEmitArgs {
    ViewSelectArgs s;               // the batch as K12a saw it (count, regions)
    const uint64_t* group_entry_base;   // exclusive scans of group_entries / group_records
    const uint64_t* group_record_base;
    int64_t store_delta;            // a record's offset in the record store = rec_off + store_delta
    uint64_t record_base, entry_base;   // selected records / entries of the batches before
    uint64_t* off;                  // [record_base + ...) of the selected records, in file order
    uint32_t* len;
    uint64_t* entry_key;            // [entry_base + ...): the region index of every entry, file order then listed order;
    uint32_t* entry_rec;            //                     its record ordinal.  Both null when regions_merged or n_regions == 0
};
// K12b
void launch_view_emit(const ViewEmitArgs& a, hipStream_t stream);
// d_perm[i] = d_entry_rec[d_order[i]], i < n
void launch_view_compose(const uint32_t* d_entry_rec, const uint32_t* d_order, uint64_t n, uint32_t* d_perm, hipStream_t stream);


// K12c, the order check of the indexed view: one lane per described record of a batch, in file order.  A record with a reference
// whose (ref_id, pos) lies in front of that of the record before it -- of `prev_key` for the batch's first record: order_key of the
// last record of the batch before, 0 for none -- sets *unsorted to 1.  Records without a reference take no part, as in the
// reference's index builder.  *last_key receives the key of the batch's last record (0 when it has no reference).
inline uint64_t view_order_key(int32_t ref, int32_t pos) {
    return ref < 0 ? 0ull : ((uint64_t)((uint32_t)ref + 1u) << 32) | (uint32_t)(pos + 1);
}
void launch_view_order(const RecDesc* d_desc, const int32_t* d_rec_ref, uint64_t n, uint64_t prev_key, uint32_t* d_unsorted,
                       unsigned long long* d_last_key, hipStream_t stream);

}  // namespace sbx
