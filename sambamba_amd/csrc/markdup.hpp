// markdup.hpp -- launchers of K10 (markdup.hip): the device side of `sambamba markdup`.
#pragma once
#include "kernels.hpp"

namespace sbx {

constexpr uint32_t kMdNone = 0xFFFFFFFFu;                       // "no mate" / "no record" in the 32-bit record-number arrays
enum MdClass : uint8_t { kMdOut = 0, kMdFragment = 1, kMdPairable = 2 };
// words of the accumulators K10 adds to
enum MdAcc : uint32_t { kMdAccBad = 0, kMdAccBytes = 1, kMdAccOr = 2, kMdAccAnd = 3, kMdAccUnmatched = 4, kMdAccDup = 5, kMdAccWords = 6 };

struct LibTable {                   // read-group id strings -> library id (ReadGroupIndex, markdup.d:659-696)
    const char* ids;                // concatenated NUL-terminated ids
    const uint32_t* id_off;         // [n_rg]
    const int32_t* library_of;      // [n_rg]
    int32_t n_rg;
};

// per record of the file, in file order (record number = index)
struct MdRecords {
    uint64_t* off;                  // offset in the record store
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

}  // namespace sbx
