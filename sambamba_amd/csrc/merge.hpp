// merge.hpp -- launchers of K11 (merge.hip): the device side of `sambamba merge` -- the records of one input rewritten on their way
// into the resident record store.
#pragma once
#include "kernels.hpp"
#include "sort.hpp"

namespace sbx {

constexpr uint32_t kMergeNone = 0xFFFFFFFFu;        // "no patch" in MergeBatch::patch_entry

// words of the accumulators: the first five are K9a's (sort.hpp SortAcc), so an input on the fast path adds to the same words
enum MergeAcc : uint32_t { kMergeAccRewritten = kSortAccWords, kMergeAccOldBytes = kSortAccWords + 1, kMergeAccWords = kSortAccWords + 2 };

// One renamed @RG / @PG id of an input.  The table of an input holds only the ids that change; ids are compared byte for byte.
struct RenameEntry {
    uint32_t old_off, old_len;      // in RenameTable::blob (no terminator)
    uint32_t new_off, new_len;
    uint32_t kind;                  // 0: RG, 1: PG
};
struct RenameTable {
    const RenameEntry* entry;
    const char* blob;
    uint32_t n;
};

// per record of ONE batch, in batch order (scratch of K11; the arrays of the whole file are K9a's key / off / len)
struct MergeBatch {
    uint32_t* new_len;              // [n] length of the rewritten record (block_size + 4); 0: the record takes no part
    uint32_t* keep;                 // [n] 1: the record takes part
    uint64_t* key;                  // [n] sort key of the rewritten record
    uint32_t* patch_at;             // [2 n] offset of the old value inside the record
    uint32_t* patch_entry;          // [2 n] its RenameEntry, kMergeNone: no (further) patch; ascending patch_at
    uint64_t* len_base;             // [n + 1] exclusive scan of new_len: offsets behind the store's fill; [n]: the batch's bytes
    uint64_t* keep_base;            // [n + 1] exclusive scan of keep: record numbers behind those of the batches before
    uint64_t* tile_sum;             // [len_tiles(n) + 2] scratch of the scans
};

struct MergeArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records
    uint64_t n;
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    int32_t n_ref_own, n_ref_merged;
    const int32_t* ref_map;         // [n_ref_own] the input's reference id -> merged id
    RenameTable table;
    uint32_t use_filter;            // != 0: only records with RecDesc::pad == kFilterPass take part (IndexArgs::filter_every)
    MergeBatch b;
    unsigned long long* acc;        // [kMergeAccWords]
    // K11b only
    uint8_t* store;
    uint64_t store_at;              // bytes of the store in use: the batch's records go behind them
    uint64_t out_base;              // records kept before this batch
    uint64_t* key;                  // arrays of the whole merge, [out_base + ...)
    uint64_t* off;
    uint32_t* len;
};
constexpr uint32_t kMergeThreads = 256;
// K11a: every record of the batch checked and described, then the two scans (MergeBatch::len_base, keep_base)
void launch_merge_describe(const MergeArgs& a, hipStream_t stream);
// K11b: the records that take part go to store + store_at + len_base[i], rewritten.  The caller has compared len_base[n] with what
// is left of the store.  store == nullptr (the key pass of the windowed merge): no byte is moved; key[r] and len[r] -- the NEW
// length -- of the records that take part are written at their ordinals out_base + keep_base[i], one lane per record, and `off`
// is not touched.
void launch_merge_rewrite(const MergeArgs& a, hipStream_t stream);

// K11c: the windowed merge (no record store).  The batch has gone through launch_merge_describe again in THIS pass (a.b is this
// pass's; a.store, a.key, a.off, a.len are not used).  The record i that takes part has the ordinal first_kept + keep_base[i]; the
// bytes of the rewritten record that lie in [w0, w1) of the merged stream go to window + (dest[ordinal] - w0) (mergewin_core.hpp).
// acc: the words of K9d-3 (sort.hpp WindowAcc) -- bytes written; records whose new length is not len[ordinal], or every record
// that takes part in THIS pass when the batch keeps another number of records than n_kept (a batch that keeps none now counts
// no record: the bytes the window then misses report it).
struct MergeWindowArgs {
    uint64_t first_kept, n_kept;    // ordinals the key pass gave the batch's records that take part: [first_kept, first_kept + n_kept)
    const uint64_t* dest;           // [ordinal] offset in the merged stream (K9d-1)
    const uint32_t* len;            // [ordinal] the new length as the key pass computed it
    uint64_t w0, w1;                // the window of the merged stream
    uint8_t* window;                // [w1 - w0]
    unsigned long long* acc;        // [kWindowAccWords]
};
void launch_merge_window_scatter(const MergeArgs& a, const MergeWindowArgs& w, hipStream_t stream);

}  // namespace sbx
