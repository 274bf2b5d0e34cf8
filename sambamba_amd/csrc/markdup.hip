// markdup.hip -- K10: the device side of `sambamba markdup` (sambamba/markdup.d).
//
//   K10a k_md_ends          one lane per record of a batch, next to the copy into the record store: the record's offset and length, its
//                           class (out / fragment / pairable), and for the records that take part the position key (library, ref_id,
//                           5' coordinate, strand), the score and -- pairable ones -- the hash of name + RG (markdup_core.hpp).  Every
//                           length the record states is checked against its block_size and the batch before a byte behind the
//                           fixed part is read (read_record_frame, wave_prims.hpp); a record that fails is counted and the call
//                           ends with SBX_EFORMAT.
//   K10b k_md_pair_runs     the pairable records, sorted by hash (K9b, stable: runs of equal hashes are in file order).  The lane at
//                           the head of a run pairs the records of the run whose name and RG BYTES are equal, 1st with 2nd, 3rd with
//                           4th; a run of two -- the usual case -- is one comparison.
//   K10c k_md_pair_keys /   pair entries in file order of their earlier record, sorted by (w0, w1, w2) word by word (LSD, a key
//        k_md_pair_dups /   gather between the words): not the head of a (w0, w1) group <=> duplicate.  Single ends and one marker
//        k_md_single_*      per end of every pair, sorted by (position key, single_word): markers and unmatched reads come first, so
//                           a fragment is a duplicate <=> it is not the first entry of its position.  Both tests look at the
//                           neighbour in sorted order only: a group may be of any size.
//   K10d k_md_patch_flags   the flag of every record in the store gets 0x400 set or cleared, byte stores at any address.
// The streamed path (a file whose records do not stay on the device; engine_markdup.cpp) has no record store:
//   K10e k_md_key_measure / per batch, next to K10a: the flag of every record as read, and for every pairable record the bytes K10b
//        k_md_key_emit      compares -- l_read_name, the name, the RG value, NUL (markdup_core.hpp) -- in a compact key store; K10b
//                           runs over those entries (k_md_pair_runs<true>).
//        k_md_out_plan      flag as read + duplicate bit -> the high flag byte to write and the length in the output (0: dropped).
//   K10f k_md_window_scatter  the records of a replayed batch go to their place in a window of the output stream, byte 19 patched.
#include "common.hpp"
#include "markdup.hpp"
#include "markdup_core.hpp"
#include "sort.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// the RG:Z value among the aux fields [t, e) of a record at `rec`: its offset from rec, *len its length; 0: none
__device__ uint32_t find_rg(const uint8_t* rec, uint64_t t, uint64_t e, uint32_t* len) {
    while (t + 3 <= e) {
        const uint8_t k0 = rec[t], k1 = rec[t + 1], ty = rec[t + 2];
        t += 3;
        const uint64_t v = t;
        switch (ty) {
            case 'A': case 'c': case 'C': t += 1; break;
            case 's': case 'S': t += 2; break;
            case 'i': case 'I': case 'f': t += 4; break;
            case 'Z': case 'H': while (t < e && rec[t]) ++t; ++t; break;
            case 'B': {
                if (t + 5 > e) return 0;
                const uint8_t sub = rec[t];
                const uint32_t n = ld32(rec + t + 1);
                const uint32_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : 4u;
                t += 5 + (uint64_t)n * w;
                break;
            }
            default: return 0;
        }
        if (k0 == 'R' && k1 == 'G') {
            if (ty != 'Z' || t > e) return 0;                // (t > e: the string is not terminated inside the record)
            *len = (uint32_t)(t - 1 - v);
            return (uint32_t)v;
        }
    }
    return 0;
}

// ---- K10a -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMdThreads) void k_md_ends(MdEndsArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    const bool live = i < a.n;
    bool bad = false;
    uint32_t len = 0;
    if (live) {
        const uint64_t rec_off = a.desc[i].rec_off, at = a.out_base + i;
        const uint8_t* p = a.U + rec_off;
        uint8_t cls = kMdOut;
        uint64_t key = 0, hash = 0;
        uint32_t score = 0, rg_at = 0;
        RecordFrame f;
        bad = !read_record_frame(a.U, rec_off, a.u_end, a.n_ref, &f);
        if (!bad) {
            len = f.bs + 4u;
            if (f.ref != -1 && !(f.flag & 0x904u)) {
                const bool reversed = f.flag & 0x10u;
                const uint64_t seq = (uint64_t)f.l_seq;
                cls = ((f.flag & 1u) && !(f.flag & 8u)) ? kMdPairable : kMdFragment;
                const uint8_t* cigar = p + 36 + f.l_name;
                const int32_t coord = mdc::five_prime_coord(f.pos, reversed, cigar, f.n_cigar);
                score = mdc::score_of(cigar + 4ull * f.n_cigar + (seq + 1) / 2, (uint32_t)seq);
                uint32_t rg_len = 0;
                rg_at = find_rg(p, 4 + f.fixed, 4ull + f.bs, &rg_len);
                int32_t library = -1;
                if (rg_at) {
                    for (int32_t g = 0; g < a.lib.n_rg; ++g) {
                        const char* id = a.lib.ids + a.lib.id_off[g];
                        uint32_t k = 0;
                        while (k < rg_len && id[k] && (uint8_t)id[k] == p[rg_at + k]) ++k;
                        if (k == rg_len && id[k] == 0) { library = a.lib.library_of[g]; break; }
                    }
                }
                key = mdc::pos_key(library, f.ref, coord, reversed ? 1u : 0u, a.ref_bits);
                if (cls == kMdPairable) hash = mdc::pair_hash(p + 36, f.l_name ? f.l_name - 1u : 0u, p + rg_at, rg_len) & a.hash_mask;
            }
        }
        a.r.off[at] = (uint64_t)((int64_t)rec_off + a.store_delta);
        a.r.len[at] = len;
        a.r.cls[at] = cls;
        a.r.pos_key[at] = key;
        a.r.score[at] = score;
        a.r.hash[at] = hash;
        a.r.rg_at[at] = rg_at;
    }
    const unsigned long long mb = __ballot(bad);
    const unsigned long long bytes = wave_sum<unsigned long long>(len);
    if ((threadIdx.x & 63u) == 0) {
        if (bytes) atomicAdd(a.acc + kMdAccBytes, bytes);
        if (mb) atomicAdd(a.acc + kMdAccBad, (unsigned long long)__popcll(mb));
    }
}

// ---- compaction: the record numbers that satisfy a predicate, in file order (block_rank_of_kept, wave_prims.hpp; the workgroups
// through launch_count_scan over k_md_compact_count's counts) ------------------------------------------------------------------
__device__ __forceinline__ bool md_pred(uint32_t pred, const uint8_t* c, const uint32_t* mate, uint64_t i) {
    switch (pred) {
        case kMdPredPairable: return c[i] == kMdPairable;
        case kMdPredPairFirst: return c[i] == kMdPairable && mate[i] != kMdNone && mate[i] > i;
        case kMdPredSingle: return c[i] == kMdFragment || (c[i] == kMdPairable && mate[i] == kMdNone);
        default: return c[i] != 0;
    }
}

__global__ __launch_bounds__(kMdThreads) void k_md_compact_count(uint32_t pred, const uint8_t* __restrict__ c, const uint32_t* __restrict__ mate,
                                                                 uint64_t n, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wcnt[kMdThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    uint32_t total;
    block_rank_of_kept(i < n && md_pred(pred, c, mate, i), wcnt, &total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kMdThreads) void k_md_compact_write(uint32_t pred, const uint8_t* __restrict__ c, const uint32_t* __restrict__ mate,
                                                                 uint64_t n, const uint64_t* __restrict__ group_base, uint32_t* __restrict__ out) {
    __shared__ uint32_t wcnt[kMdThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    const bool keep = i < n && md_pred(pred, c, mate, i);
    const uint32_t rank = block_rank_of_kept(keep, wcnt);
    if (keep) out[group_base[blockIdx.x] + rank] = (uint32_t)i;
}

__global__ __launch_bounds__(kMdThreads) void k_md_gather_keys(const uint64_t* __restrict__ word, const uint32_t* __restrict__ idx, uint64_t n,
                                                               uint64_t* __restrict__ key, unsigned long long* __restrict__ acc) {
    const uint64_t j = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    const bool live = j < n;
    const uint64_t k = live ? word[idx[j]] : 0;
    if (live) key[j] = k;
    const unsigned long long k_or = wave_or(live ? k : 0ull), k_and = wave_and(live ? k : ~0ull);
    if ((threadIdx.x & 63u) == 0 && live) {               // (lane 0 is live when any lane of the wave is)
        atomicOr(acc + kMdAccOr, k_or);
        atomicAnd(acc + kMdAccAnd, k_and);
    }
}

// ---- K10b -----------------------------------------------------------------------------------------------------------------
// name and RG string of two records of the store, byte for byte (readsArePaired; an absent RG is the empty string)
__device__ bool md_same_key(const uint8_t* store, const MdRecords& r, uint32_t x, uint32_t y) {
    const uint8_t* p = store + r.off[x];
    const uint8_t* q = store + r.off[y];
    const uint32_t ln = p[12];
    if (ln != q[12]) return false;
    for (uint32_t k = 0; k < ln; ++k) if (p[36 + k] != q[36 + k]) return false;
    const uint32_t ax = r.rg_at[x], ay = r.rg_at[y], ex = r.len[x], ey = r.len[y];
    // (K10a found both strings terminated inside their records)
    uint32_t k = 0;
    for (;; ++k) {
        const uint8_t cx = ax && ax + k < ex ? p[ax + k] : 0, cy = ay && ay + k < ey ? q[ay + k] : 0;
        if (cx != cy) return false;
        if (!cx) return true;
    }
}

// the key store's reader of the same comparison (the streamed path): the entries K10e wrote, r.off[record] their offsets
__device__ bool md_same_entry(const uint8_t* keys, const MdRecords& r, uint32_t x, uint32_t y) {
    return mdc::pair_keys_equal(keys + r.off[x], keys + r.off[y]);
}

// kKeyStore: `store` is the key store and md_same_entry compares; otherwise the record store and md_same_key
template <bool kKeyStore>
__global__ __launch_bounds__(kMdThreads) void k_md_pair_runs(const uint64_t* __restrict__ hash, const uint32_t* __restrict__ rec, uint64_t n,
                                                             const uint8_t* __restrict__ store, MdRecords r, uint32_t* mate) {
    const uint64_t j = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    if (j >= n) return;
    const uint64_t h = hash[j];
    if (j > 0 && hash[j - 1] == h) return;               // not the head of its run
    uint64_t e = j + 1;
    while (e < n && hash[e] == h) ++e;
    if (e == j + 1) return;
    for (uint64_t x = j; x + 1 < e; ++x) {
        const uint32_t rx = rec[x];
        if (mate[rx] != kMdNone) continue;
        for (uint64_t y = x + 1; y < e; ++y) {
            const uint32_t ry = rec[y];
            if (mate[ry] != kMdNone || !(kKeyStore ? md_same_entry(store, r, rx, ry) : md_same_key(store, r, rx, ry))) continue;
            mate[rx] = ry;
            mate[ry] = rx;
            break;
        }
    }
}

// ---- K10c -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMdThreads) void k_md_pair_keys(const uint32_t* __restrict__ first, const uint32_t* __restrict__ mate, uint64_t n_pairs,
                                                             MdRecords r, uint32_t ref_bits, uint64_t* __restrict__ w0, uint64_t* __restrict__ w1,
                                                             uint64_t* __restrict__ w2, uint64_t* __restrict__ end2) {
    const uint64_t e = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    if (e >= n_pairs) return;
    const uint32_t x = first[e], y = mate[x];
    uint64_t w[3], k2;
    mdc::pair_words(r.pos_key[x], r.score[x], r.pos_key[y], r.score[y], ref_bits, w, &k2);
    w0[e] = w[0]; w1[e] = w[1]; w2[e] = w[2]; end2[e] = k2;
}

__global__ __launch_bounds__(kMdThreads) void k_md_pair_dups(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ w0,
                                                             const uint64_t* __restrict__ w1, uint64_t n_pairs, const uint32_t* __restrict__ first,
                                                             const uint32_t* __restrict__ mate, uint8_t* __restrict__ dup) {
    const uint64_t j = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    if (j >= n_pairs || j == 0) return;
    const uint32_t e = perm[j], f = perm[j - 1];
    if (w0[e] != w0[f] || w1[e] != w1[f]) return;         // the head of its group: the best pair
    const uint32_t x = first[e];
    dup[x] = 1;
    dup[mate[x]] = 1;
}

__global__ __launch_bounds__(kMdThreads) void k_md_single_entries(const uint64_t* __restrict__ w0, const uint64_t* __restrict__ end2, uint64_t n_pairs,
                                                                  const uint32_t* __restrict__ single, uint64_t n_single, MdRecords r,
                                                                  uint64_t* __restrict__ v0, uint64_t* __restrict__ v1, uint32_t* __restrict__ rec,
                                                                  unsigned long long* __restrict__ acc) {
    const uint64_t e = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    bool unmatched = false;
    if (e < 2 * n_pairs) {
        v0[e] = (e & 1) ? end2[e >> 1] : w0[e >> 1];
        v1[e] = 0;
        rec[e] = kMdNone;
    } else if (e < 2 * n_pairs + n_single) {
        const uint32_t x = single[e - 2 * n_pairs];
        const bool fragment = r.cls[x] == kMdFragment;
        unmatched = !fragment;
        v0[e] = r.pos_key[x];
        v1[e] = mdc::single_word(fragment, r.score[x]);
        rec[e] = x;
    }
    const unsigned long long m = __ballot(unmatched);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(acc + kMdAccUnmatched, (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kMdThreads) void k_md_single_dups(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ v0,
                                                               const uint64_t* __restrict__ v1, const uint32_t* __restrict__ rec, uint64_t m,
                                                               uint8_t* __restrict__ dup) {
    const uint64_t j = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    if (j >= m || j == 0) return;
    const uint32_t e = perm[j];
    if (!(v1[e] & mdc::kFragmentBit) || v0[e] != v0[perm[j - 1]]) return;
    dup[rec[e]] = 1;
}

// ---- K10d -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMdThreads) void k_md_patch_flags(uint8_t* __restrict__ store, const uint64_t* __restrict__ off,
                                                               const uint8_t* __restrict__ dup, uint64_t n, uint32_t remove, uint8_t* __restrict__ keep,
                                                               unsigned long long* __restrict__ acc) {
    const uint64_t i = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    bool marked = false;
    if (i < n) {
        uint8_t* f = store + off[i] + 18;                 // flag: bytes 18-19 of the record, block_size included
        marked = dup[i] != 0;
        const uint32_t flag = mdc::flag_after(f[0] | (uint32_t)f[1] << 8, marked);
        f[1] = (uint8_t)(flag >> 8);                      // (0x400 lives in the high byte)
        keep[i] = mdc::kept(flag, remove != 0);
    }
    const unsigned long long m = __ballot(marked);
    if ((threadIdx.x & 63u) == 0 && m) atomicAdd(acc + kMdAccDup, (unsigned long long)__popcll(m));
}

// ---- K10e: the key store of the streamed path ---------------------------------------------------------------------------------
// Nothing is read that K10a's checks did not cover: a record K10a refused has len 0 and is left alone; the flag lies in the fixed
// part; the RG value was found terminated inside the record (find_rg), and the walk to its NUL stops at the record's end anyway.
__global__ __launch_bounds__(kMdThreads) void k_md_key_measure(MdKeyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint64_t at = a.out_base + i;
    const uint32_t len = a.r.len[at];
    uint32_t flag = 0, klen = 0;
    if (len) {
        const uint8_t* p = a.U + a.desc[i].rec_off;
        flag = p[18] | (uint32_t)p[19] << 8;
        if (a.r.cls[at] == kMdPairable) {
            const uint32_t rg_at = a.r.rg_at[at];
            uint32_t rg_len = 0;
            if (rg_at) while (rg_at + rg_len < len && p[rg_at + rg_len]) ++rg_len;
            klen = mdc::pair_key_len(p[12], rg_len);
        }
    }
    a.flag[at] = (uint16_t)flag;
    a.key_len[i] = klen;
}

__global__ __launch_bounds__(kMdThreads) void k_md_key_emit(MdKeyArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * (kMdThreads / kCopyGroup) + threadIdx.x / kCopyGroup;
    const uint32_t l = threadIdx.x % kCopyGroup;
    if (i >= a.n) return;
    const uint32_t klen = a.key_len[i];
    if (!klen) return;
    const uint64_t at = a.out_base + i, ko = a.key_off[i];
    const uint8_t* p = a.U + a.desc[i].rec_off;
    const uint32_t l_name = p[12], rg_at = a.r.rg_at[at], rg_len = klen - 2u - l_name;
    uint8_t* dst = a.key_store + ko;
    for (uint32_t k = l; k < klen; k += kCopyGroup) dst[k] = mdc::pair_key_byte(p, l_name, rg_at, rg_len, k);
    if (l == 0) a.r.off[at] = ko;
}

// ---- the output plan of the streamed path -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMdThreads) void k_md_out_plan(const uint16_t* __restrict__ flag, const uint8_t* __restrict__ dup,
                                                            const uint32_t* __restrict__ len, uint64_t n, uint32_t remove,
                                                            uint8_t* __restrict__ hi, uint32_t* __restrict__ out_len,
                                                            unsigned long long* __restrict__ acc) {
    __shared__ uint32_t wsum[kMdThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kMdThreads + threadIdx.x;
    uint32_t marked = 0, keep = 0;
    if (i < n) {
        marked = dup[i] != 0;
        const uint32_t f = mdc::flag_after(flag[i], marked != 0);
        keep = mdc::kept(f, remove != 0);
        hi[i] = (uint8_t)(f >> 8);
        out_len[i] = keep ? len[i] : 0u;
    }
    const uint32_t n_marked = block_sum(marked, wsum), n_keep = block_sum(keep, wsum);
    if (threadIdx.x == 0) {
        if (n_marked) atomicAdd(acc + kMdAccDup, (unsigned long long)n_marked);
        if (n_keep) atomicAdd(acc + kMdAccKept, (unsigned long long)n_keep);
    }
}

// ---- K10f -------------------------------------------------------------------------------------------------------------------------
// Sixteen lanes per record, kMdScatterRounds records per lane group: in every round the sixteen groups of a workgroup move sixteen
// consecutive records, whose destinations ascend with the record number, so the workgroup's stores are adjacent.  The two counts are
// summed over the workgroup (block_sum) and cost one atomic each per 64 records -- K9d-3 issues one per wave, four records.
constexpr uint32_t kMdScatterThreads = 256, kMdScatterGroups = kMdScatterThreads / kCopyGroup, kMdScatterRounds = 4;
constexpr uint32_t kMdScatterRecs = kMdScatterGroups * kMdScatterRounds;

__global__ __launch_bounds__(kMdScatterThreads) void k_md_window_scatter(MdScatterArgs a) {
    __shared__ unsigned long long wsum[kMdScatterThreads / 64];
    const uint32_t g = threadIdx.x / kCopyGroup, l = threadIdx.x % kCopyGroup;
    unsigned long long wrote = 0, bad_n = 0;
    for (uint32_t round = 0; round < kMdScatterRounds; ++round) {
        const uint64_t i = (uint64_t)blockIdx.x * kMdScatterRecs + round * kMdScatterGroups + g;
        if (i >= a.n) break;
        const uint64_t rec_off = a.desc[i].rec_off, ord = a.first + i;
        // the record as it is in THIS pass: its frame bounds the loads, the clip of [dest, dest + its length) the stores
        bool bad = rec_off + 4 > a.u_end;
        uint32_t bs = 0;
        if (!bad) { bs = ld32(a.U + rec_off); bad = !record_len_ok(bs, rec_off, a.u_end); }
        const uint64_t len = (uint64_t)bs + 4u;
        bad = bad || len != a.len[ord];
        const uint32_t out_len = a.out_len[ord];
        sortc::PieceClip c;
        const uint64_t d = a.dest[ord];
        if (!bad && out_len && sortc::clip_to_piece(d, d + len, a.w0, a.w1, &c)) {
            // bytes [s0, s1) of the record go to dst[0 ..): what lies in front of byte 19, byte 19 patched, what lies behind it
            const uint8_t* src = a.U + rec_off;
            uint8_t* dst = a.window + c.dst;
            const uint64_t s0 = c.src, s1 = c.src + c.len;
            if (s0 < 19) { const uint64_t e = s1 < 19 ? s1 : 19; copy_span16(dst, src + s0, e - s0, l); }
            if (l == 0 && s0 <= 19 && 19 < s1) dst[19 - s0] = a.hi[ord];
            if (s1 > 20) { const uint64_t b = s0 > 20 ? s0 : 20; copy_span16(dst + (b - s0), src + b, s1 - b, l); }
            if (l == 0) wrote += c.len;
        }
        if (l == 0 && bad) ++bad_n;
    }
    wrote = block_sum(wrote, wsum);
    bad_n = block_sum(bad_n, wsum);
    if (threadIdx.x == 0) {
        if (wrote) atomicAdd(a.acc + kWindowAccBytes, wrote);
        if (bad_n) atomicAdd(a.acc + kWindowAccMismatch, bad_n);
    }
}

template <class... A, class... B>
void md_launch(void (*k)(A...), uint64_t n, hipStream_t stream, B... args) {
    if (!n) return;
    hipLaunchKernelGGL(k, dim3(md_groups(n)), dim3(kMdThreads), 0, stream, args...);
    SBX_HIP(hipGetLastError());
}

}  // namespace

void launch_md_ends(const MdEndsArgs& a, hipStream_t stream) { md_launch(k_md_ends, a.n, stream, a); }

void launch_md_compact(MdPred pred, const uint8_t* d_c, const uint32_t* d_mate, uint64_t n, uint32_t* d_group_count, uint64_t* d_group_base,
                       uint32_t* d_out, hipStream_t stream) {
    if (!n) return;
    const uint32_t groups = md_groups(n);
    md_launch(k_md_compact_count, n, stream, (uint32_t)pred, d_c, d_mate, n, d_group_count);
    launch_count_scan(d_group_count, groups, d_group_base, stream);
    md_launch(k_md_compact_write, n, stream, (uint32_t)pred, d_c, d_mate, n, (const uint64_t*)d_group_base, d_out);
}

void launch_md_gather_keys(const uint64_t* d_word, const uint32_t* d_idx, uint64_t n, uint64_t* d_key, unsigned long long* d_acc, hipStream_t stream) {
    md_launch(k_md_gather_keys, n, stream, d_word, d_idx, n, d_key, d_acc);
}

void launch_md_pair_runs(const uint64_t* d_hash, const uint32_t* d_rec, uint64_t n, const uint8_t* d_store, const MdRecords& r, uint32_t* d_mate,
                         hipStream_t stream) {
    md_launch(k_md_pair_runs<false>, n, stream, d_hash, d_rec, n, d_store, r, d_mate);
}

void launch_md_pair_runs_keys(const uint64_t* d_hash, const uint32_t* d_rec, uint64_t n, const uint8_t* d_key_store, const MdRecords& r,
                              uint32_t* d_mate, hipStream_t stream) {
    md_launch(k_md_pair_runs<true>, n, stream, d_hash, d_rec, n, d_key_store, r, d_mate);
}

void launch_md_pair_keys(const uint32_t* d_first, const uint32_t* d_mate, uint64_t n_pairs, const MdRecords& r, uint32_t ref_bits, uint64_t* d_w0,
                         uint64_t* d_w1, uint64_t* d_w2, uint64_t* d_end2, hipStream_t stream) {
    md_launch(k_md_pair_keys, n_pairs, stream, d_first, d_mate, n_pairs, r, ref_bits, d_w0, d_w1, d_w2, d_end2);
}

void launch_md_pair_dups(const uint32_t* d_perm, const uint64_t* d_w0, const uint64_t* d_w1, uint64_t n_pairs, const uint32_t* d_first,
                         const uint32_t* d_mate, uint8_t* d_dup, hipStream_t stream) {
    md_launch(k_md_pair_dups, n_pairs, stream, d_perm, d_w0, d_w1, n_pairs, d_first, d_mate, d_dup);
}

void launch_md_single_entries(const uint64_t* d_w0, const uint64_t* d_end2, uint64_t n_pairs, const uint32_t* d_single, uint64_t n_single,
                              const MdRecords& r, uint64_t* d_v0, uint64_t* d_v1, uint32_t* d_rec, unsigned long long* d_acc, hipStream_t stream) {
    md_launch(k_md_single_entries, 2 * n_pairs + n_single, stream, d_w0, d_end2, n_pairs, d_single, n_single, r, d_v0, d_v1, d_rec, d_acc);
}

void launch_md_single_dups(const uint32_t* d_perm, const uint64_t* d_v0, const uint64_t* d_v1, const uint32_t* d_rec, uint64_t m, uint8_t* d_dup,
                           hipStream_t stream) {
    md_launch(k_md_single_dups, m, stream, d_perm, d_v0, d_v1, d_rec, m, d_dup);
}

void launch_md_patch_flags(uint8_t* d_store, const uint64_t* d_off, const uint8_t* d_dup, uint64_t n, uint32_t remove, uint8_t* d_keep,
                           unsigned long long* d_acc, hipStream_t stream) {
    md_launch(k_md_patch_flags, n, stream, d_store, d_off, d_dup, n, remove, d_keep, d_acc);
}

void launch_md_key_measure(const MdKeyArgs& a, hipStream_t stream) { md_launch(k_md_key_measure, a.n, stream, a); }

void launch_md_key_emit(const MdKeyArgs& a, hipStream_t stream) {
    if (!a.n) return;
    const uint64_t per_group = kMdThreads / kCopyGroup;
    hipLaunchKernelGGL(k_md_key_emit, dim3((uint32_t)((a.n + per_group - 1) / per_group)), dim3(kMdThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_md_out_plan(const uint16_t* d_flag, const uint8_t* d_dup, const uint32_t* d_len, uint64_t n, uint32_t remove, uint8_t* d_hi,
                        uint32_t* d_out_len, unsigned long long* d_acc, hipStream_t stream) {
    md_launch(k_md_out_plan, n, stream, d_flag, d_dup, d_len, n, remove, d_hi, d_out_len, d_acc);
}

void launch_md_window_scatter(const MdScatterArgs& a, hipStream_t stream) {
    if (!a.n || a.w1 <= a.w0) return;
    hipLaunchKernelGGL(k_md_window_scatter, dim3((uint32_t)((a.n + kMdScatterRecs - 1) / kMdScatterRecs)), dim3(kMdScatterThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
