// sort.hpp -- launchers of K9 (sort.hip): the device side of `sambamba sort`, coordinate order.
#pragma once
#include "kernels.hpp"

namespace sbx {

// words of the accumulators K9a adds to over the batches of a file
enum SortAcc : uint32_t { kSortAccOr = 0, kSortAccAnd = 1, kSortAccKept = 2, kSortAccBytes = 3, kSortAccBad = 4, kSortAccWords = 5 };

struct SortKeysArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records
    const int32_t* rec_ref;
    uint64_t n;                     // records of the batch
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    int32_t n_ref;                  // reference ids of the file are in [-1, n_ref)
    int32_t key_n_ref;              // the id that stands for -1 in the key: n_ref for one file, the size of the merged dictionary in sbx_merge_bam
    uint32_t use_filter;            // != 0: only records with RecDesc::pad == kFilterPass take part (IndexArgs::filter_every)
    int64_t store_delta;            // a record's offset in the record store = rec_off + store_delta
    uint64_t out_base;              // records kept of the batches before
    uint64_t* key;                  // [out_base + ...) of the kept records, in file order
    uint64_t* off;                  // (null: no record store, the windowed sort)
    uint32_t* len;
    unsigned long long* acc;        // [kSortAccWords]
};
constexpr uint32_t kSortKeysThreads = 256;
inline uint32_t sort_keys_groups(uint64_t n) { return (uint32_t)((n + kSortKeysThreads - 1) / kSortKeysThreads); }
// K9a.  With a filter: d_group_count / d_group_base have sort_keys_groups(n) + 2 entries (the kept records per workgroup and their
// exclusive scan, which keeps the compaction in file order); without, both may be null.
void launch_sort_keys(const SortKeysArgs& a, uint32_t* d_group_count, uint64_t* d_group_base, hipStream_t stream);

// K9b: one pass of the stable LSD radix sort over the 8-bit digit at `shift`.  d_hist has radix_hist_entries(n) + 4 counters,
// d_hist_base as many + 2 offsets.
constexpr uint32_t kRadixTile = 4096;
inline uint32_t radix_tiles(uint64_t n) { return (uint32_t)((n + kRadixTile - 1) / kRadixTile); }
inline size_t radix_hist_entries(uint64_t n) { return (size_t)radix_tiles(n) * 256; }
void launch_radix_pass(const uint64_t* d_key_in, const uint32_t* d_val_in, uint64_t* d_key_out, uint32_t* d_val_out, uint64_t n, uint32_t shift,
                       uint32_t* d_hist, uint64_t* d_hist_base, hipStream_t stream);

// d_rec[k], k in [0, n_bounds): the first record that ends behind byte k * piece_bytes of the sorted stream (n: none)
void launch_piece_bounds(const uint64_t* d_out_off, uint64_t n, uint64_t piece_bytes, uint32_t n_bounds, uint32_t* d_rec, hipStream_t stream);
// K9c: the bytes of sorted records [r0, r1) that lie in [p0, p1) of the sorted stream go to d_dst[0, p1 - p0)
void launch_gather_records(const uint8_t* d_store, const uint64_t* d_off, const uint32_t* d_perm, const uint64_t* d_out_off, uint64_t r0,
                           uint64_t r1, uint64_t p0, uint64_t p1, uint8_t* d_dst, hipStream_t stream);

// ---- K9d: the windowed sort (no record store; the file passes through the read pass once per window of the output stream) ----
// K9d-1: d_dest[d_perm[r]] = d_out_off[r], r in [0, n): where in the sorted stream the kept record with file-order ordinal i starts
void launch_window_dest(const uint32_t* d_perm, const uint64_t* d_out_off, uint64_t n, uint64_t* d_dest, hipStream_t stream);
// K9d-2: batch b holds the kept records [d_first[b], d_first[b + 1]); d_lo[b] = min dest, d_hi[b] = max (dest + len) over them
// (~0 and 0 for a batch without records)
void launch_batch_spans(const uint64_t* d_dest, const uint32_t* d_len, const uint64_t* d_first, uint32_t n_batches, uint64_t* d_lo,
                        uint64_t* d_hi, hipStream_t stream);
// words of K9d-3's accumulator: bytes written into the window; records that are not what the key pass saw
enum WindowAcc : uint32_t { kWindowAccBytes = 0, kWindowAccMismatch = 1, kWindowAccWords = 2 };
struct WindowScatterArgs {
    const uint8_t* U;               // inflated bytes of the replayed batch
    const RecDesc* desc;            // its records
    uint64_t n;                     // records of the batch
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    uint32_t use_filter;            // != 0: only records with RecDesc::pad == kFilterPass take part, numbered as K9a numbered them
    uint64_t first_kept, n_kept;    // ordinals the key pass gave the batch's kept records: [first_kept, first_kept + n_kept)
    const uint64_t* dest;           // [ordinal] offset in the sorted stream (K9d-1)
    const uint32_t* len;            // [ordinal] block_size + 4 as the key pass read it
    uint64_t w0, w1;                // the window of the sorted stream
    uint8_t* window;                // [w1 - w0]
    unsigned long long* acc;        // [kWindowAccWords]
};
// K9d-3.  With a filter: d_group_count / d_group_base as for launch_sort_keys, d_rank has n + 2 words (a kept record's rank among
// the kept records of the batch); without, all three may be null.
void launch_window_scatter(const WindowScatterArgs& a, uint32_t* d_group_count, uint64_t* d_group_base, uint32_t* d_rank, hipStream_t stream);

}  // namespace sbx
