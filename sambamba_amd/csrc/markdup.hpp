// markdup.hpp -- launchers of K10 (markdup.hip): the device side of `sambamba markdup`.
#pragma once
#include "kernels.hpp"

namespace sbx {

constexpr uint32_t kMdNone = 0xFFFFFFFFu;                       // "no mate" / "no record" in the 32-bit record-number arrays
enum MdClass : uint8_t { kMdOut = 0, kMdFragment = 1, kMdPairable = 2 };
// words of the accumulators K10 adds to
enum MdAcc : uint32_t { kMdAccBad = 0, kMdAccBytes = 1, kMdAccOr = 2, kMdAccAnd = 3, kMdAccUnmatched = 4, kMdAccDup = 5, kMdAccKept = 6, kMdAccWords = 7 };

struct LibTable {                   // read-group id strings -> library id (ReadGroupIndex, markdup.d:659-696)
    const char* ids;                // concatenated NUL-terminated ids
    const uint32_t* id_off;         // [n_rg]
    const int32_t* library_of;      // [n_rg]
    int32_t n_rg;
};

// per record of the file, in file order (record number = index)
struct MdRecords {
    uint64_t* off;                  // offset in the record store; on the streamed path (no record store) K10e puts the offset of a
                                    // pairable record's entry in the key store here instead -- other records' values mean nothing there
    uint32_t* len;                  // block_size + 4
    uint8_t* cls;                   // MdClass
    uint64_t* pos_key;              // markdup_core.hpp pos_key (class != out)
    uint32_t* score;
    uint64_t* hash;                 // pair_hash (pairable records)
    uint32_t* rg_at;                // offset of the RG:Z value inside the record, 0: none
};

struct MdEndsArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records
    uint64_t n;
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    int32_t n_ref;
    uint32_t ref_bits;
    uint64_t hash_mask;             // SBX_MARKDUP_HASH_BITS (all ones otherwise)
    int64_t store_delta;            // a record's offset in the record store = rec_off + store_delta
    uint64_t out_base;              // records of the batches before
    LibTable lib;
    MdRecords r;
    unsigned long long* acc;        // [kMdAccWords]
};
// K10a: one descriptor per record of a batch
void launch_md_ends(const MdEndsArgs& a, hipStream_t stream);

// Stable compaction of the record numbers [0, n) that satisfy a predicate, in ascending order (the K9a pattern: counts per workgroup,
// their exclusive scan, ballot + prefix inside).  d_group_count / d_group_base: md_groups(n) + 4 entries.  d_group_base[md_groups(n)]
// receives the number of entries written.
enum MdPred : uint32_t { kMdPredPairable = 0, kMdPredPairFirst = 1, kMdPredSingle = 2, kMdPredKeep = 3 };
constexpr uint32_t kMdThreads = 256;
inline uint32_t md_groups(uint64_t n) { return (uint32_t)((n + kMdThreads - 1) / kMdThreads); }
void launch_md_compact(MdPred pred, const uint8_t* d_cls_or_keep, const uint32_t* d_mate, uint64_t n, uint32_t* d_group_count,
                       uint64_t* d_group_base, uint32_t* d_out, hipStream_t stream);

// d_key[j] = d_word[d_idx[j]] for j < n; ORs / ANDs them into acc[kMdAccOr / kMdAccAnd] (the digits a radix sort may skip)
void launch_md_gather_keys(const uint64_t* d_word, const uint32_t* d_idx, uint64_t n, uint64_t* d_key, unsigned long long* d_acc, hipStream_t stream);

// K10b: (d_hash, d_rec) sorted by hash, runs in file order.  Inside a run of equal hashes the records whose name and RG bytes are equal
// pair up 1st with 2nd, 3rd with 4th ...: d_mate[record] = its partner (kMdNone stays for a leftover).
void launch_md_pair_runs(const uint64_t* d_hash, const uint32_t* d_rec, uint64_t n, const uint8_t* d_store, const MdRecords& r, uint32_t* d_mate,
                         hipStream_t stream);
// The same runs for the streamed path: r.off[record] is the offset of the record's entry in d_key_store (K10e) and two records are
// equal when their entries are (mdc::pair_keys_equal).  r.len and r.rg_at are not read.
void launch_md_pair_runs_keys(const uint64_t* d_hash, const uint32_t* d_rec, uint64_t n, const uint8_t* d_key_store, const MdRecords& r,
                              uint32_t* d_mate, hipStream_t stream);

// K10c, pairs: entry e is the pair whose earlier record is d_first[e]; its key words go to d_w0 / d_w1 / d_w2, the position key of
// its second end to d_end2
void launch_md_pair_keys(const uint32_t* d_first, const uint32_t* d_mate, uint64_t n_pairs, const MdRecords& r, uint32_t ref_bits, uint64_t* d_w0,
                         uint64_t* d_w1, uint64_t* d_w2, uint64_t* d_end2, hipStream_t stream);
// d_perm: the pair entries sorted by (w0, w1, w2), stable.  Every pair that is not the first of its (w0, w1) group has both records marked.
void launch_md_pair_dups(const uint32_t* d_perm, const uint64_t* d_w0, const uint64_t* d_w1, uint64_t n_pairs, const uint32_t* d_first,
                         const uint32_t* d_mate, uint8_t* d_dup, hipStream_t stream);
// K10c, single ends: entries [0, 2 n_pairs) are the markers of the pairs' ends, [2 n_pairs, 2 n_pairs + n_single) the single ends
// d_single[]; d_v0 = position key, d_v1 = single_word, d_rec = record number (kMdNone for a marker).  Counts the unmatched reads.
void launch_md_single_entries(const uint64_t* d_w0, const uint64_t* d_end2, uint64_t n_pairs, const uint32_t* d_single, uint64_t n_single,
                              const MdRecords& r, uint64_t* d_v0, uint64_t* d_v1, uint32_t* d_rec, unsigned long long* d_acc, hipStream_t stream);
// d_perm: the entries sorted by (v0, v1), stable.  A fragment that is not the first entry of its v0 group is marked.
void launch_md_single_dups(const uint32_t* d_perm, const uint64_t* d_v0, const uint64_t* d_v1, const uint32_t* d_rec, uint64_t m, uint8_t* d_dup,
                           hipStream_t stream);

// K10d: the duplicate bit of every record goes into its flag in the store (markdup.d:1286-1292); d_keep[i] = the record is written
// (always without `remove`); acc[kMdAccDup] += marked records
void launch_md_patch_flags(uint8_t* d_store, const uint64_t* d_off, const uint8_t* d_dup, uint64_t n, uint32_t remove, uint8_t* d_keep,
                           unsigned long long* d_acc, hipStream_t stream);

// ---- the streamed path: no record store; the file passes through the read pass once more while the output is written ----
// K10e, per batch, right after K10a (same U, same descriptors; a.r holds K10a's results for the batch at a.out_base).
struct MdKeyArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records
    uint64_t n;
    uint64_t out_base;              // records of the batches before
    MdRecords r;                    // len, cls, rg_at are read (len 0: K10a refused the record, nothing of it is read); off is written
    uint16_t* flag;                 // [record number] the record's flag as read
    uint32_t* key_len;              // [n + 2], of the batch: bytes of the record's entry (0: not pairable)
    uint64_t* key_off;              // [n + 2], of the batch: where the entry starts in the key store (the scan of key_len)
    uint8_t* key_store;
};
// K10e-1: the flag of every record and the length of every pairable record's entry, one lane per record
void launch_md_key_measure(const MdKeyArgs& a, hipStream_t stream);
// K10e-2: the entries (mdc::pair_key_byte), sixteen lanes per record; r.off[record] = key_off of a pairable record
void launch_md_key_emit(const MdKeyArgs& a, hipStream_t stream);

// The output plan: from the flag as read and d_dup, d_hi[i] = the high flag byte the record is written with (mdc::flag_after) and
// d_out_len[i] = the record's length when it is written (mdc::kept), 0 otherwise; acc[kMdAccDup] += marked records, acc[kMdAccKept]
// += records written.  One atomic per workgroup and word.
void launch_md_out_plan(const uint16_t* d_flag, const uint8_t* d_dup, const uint32_t* d_len, uint64_t n, uint32_t remove, uint8_t* d_hi,
                        uint32_t* d_out_len, unsigned long long* d_acc, hipStream_t stream);

// K10f (md_window_scatter): sixteen lanes per record of a replayed batch.  A record that is written (out_len != 0) is clipped to the
// window [w0, w1) of the output stream and copied to window + dest - w0; byte 19 of the record -- the high flag byte -- receives
// hi[record] when it lies in the window (a record may straddle two windows: the byte is written once, by the window that owns it).
// Every record's length in this pass is compared with the one the key pass read, written or not.  acc (WindowAcc, sort.hpp):
// bytes written and mismatches, summed per workgroup, one atomic per workgroup and word.
struct MdScatterArgs {
    const uint8_t* U;               // inflated bytes of the replayed batch
    const RecDesc* desc;            // its records
    uint64_t n;                     // records of the batch
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    uint64_t first;                 // record number of the batch's first record
    const uint64_t* dest;           // [record number] offset in the output stream
    const uint32_t* len;            // [record number] block_size + 4 as the key pass read it
    const uint32_t* out_len;        // [record number] len, or 0 for a record that is not written
    const uint8_t* hi;              // [record number] the high flag byte to write
    uint64_t w0, w1;                // the window of the output stream
    uint8_t* window;                // [w1 - w0]
    unsigned long long* acc;        // [kWindowAccWords]
};
void launch_md_window_scatter(const MdScatterArgs& a, hipStream_t stream);

}  // namespace sbx
