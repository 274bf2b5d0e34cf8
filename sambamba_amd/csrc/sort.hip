// sort.hip -- K9: the device side of `sambamba sort` in coordinate order (sambamba/sort.d, default mode).
//
//   K9a  k_sort_keys      one lane per described record of a batch: the 64-bit key (sort_core.hpp) from rec_ref, RecDesc::pos and
//                         RecDesc::flag, the record's length (block_size + 4, read from U at any byte address) and its offset in the
//                         resident record store.  With -F the records the filter rejects (RecDesc::pad, written by K2) are compacted
//                         away: inside a workgroup by block_rank_of_kept (wave_prims.hpp), the workgroups through an exclusive scan
//                         of their counts (k_sort_group_count) -- so the kept records stay in file order, which is what makes the
//                         sort below stable with respect to the file.  The kernel also folds the keys into an OR and an AND word:
//                         the bits in which two keys of the file differ are the only ones K9b has to sort.
//   K9b  k_radix_hist /   stable LSD radix sort of (key, record number), 8 bits per pass.  A workgroup of four waves owns a tile of
//        k_radix_scatter  4096 consecutive elements and takes them in sixteen rounds of 256.  Histogram: LDS atomics, one counter row
//                         per tile, laid out [digit][tile] so that one exclusive scan (launch_count_scan) yields the first output
//                         slot of every (digit, tile).  Scatter: inside a wave the lanes with the same digit find one another with
//                         eight ballots (one per digit bit); the lane's rank among them is a popcount below its own lane, the lowest
//                         of them publishes the count in the wave's row of LDS, and a lane's slot is the tile's running offset of its
//                         digit + the counts of the waves in front + its rank -- input order, hence stable.  No atomics in the scatter.
//   K9c  k_gather_records sixteen lanes per record: the record's bytes go from the store to their place in a piece of the sorted
//                         stream, both ends at arbitrary byte addresses (copy_span16, wave_prims.hpp).  A piece is a whole number
//                         of BGZF payloads; a record that straddles a piece boundary is copied in part by both pieces.
//
//   K9d  the windowed sort: a file whose records do not fit the device has no record store.  Only its keys are sorted; the sorted
//        stream is written window by window (sort_core.hpp: window_at), and for every window the file passes through K1 + K2 again.
//     K9d-1  k_window_dest     one lane per sorted rank r: dest[perm[r]] = out_off[r] -- where the kept record with file-order
//                              ordinal i starts in the sorted stream.  Keys, permutation and offsets are released after it.
//     K9d-2  k_batch_spans     one workgroup per batch of the read pass: the minimum of dest and the maximum of dest + len over the
//                              batch's ordinals (wave_min / wave_max, the waves through LDS).  A window replays only the batches
//                              whose span meets it.
//     K9d-3  k_window_scatter  sixteen lanes per described record of a replayed batch, the shape of K9c: the record's ordinal is
//                              the batch's saved first ordinal + its index, with -F + its rank among the kept records
//                              (k_window_rank: block_rank_of_kept + the scan of k_sort_group_count, the numbering of K9a); its
//                              bytes, clipped to the window [w0, w1) with the length READ IN THIS PASS, go from U to
//                              window + (dest - w0).  The clip is what bounds the stores.  Every wave adds the bytes it wrote to a
//                              64-bit counter and the records whose length is not the saved one (or that have no saved ordinal)
//                              to a second: the host refuses the window unless the first is the window's record bytes and the
//                              second 0.
//
// Bytes moved (n records, b bytes of records): K9a reads 36 n (descriptor, rec_ref) + 4 n scattered words of U and writes 20 n; a pass of
// K9b reads 12 n twice (histogram: keys only, 8 n) and writes 12 n; the offsets (scan.hip) read 8 n and write 8 n; K9c reads and writes b.
// K9d-1 reads 12 n and writes 8 n (scattered); K9d-2 reads 12 n; K9d-3, for a window of w bytes filled from batches of r records,
// reads 48 r (descriptor, block_size, saved length, dest; with -F 4 r more, written and read) + w and writes w.
#include "common.hpp"
#include "sort.hpp"
#include "sort_core.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// ---- K9a -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSortKeysThreads) void k_sort_group_count(const RecDesc* __restrict__ desc, uint64_t n, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wcnt[kSortKeysThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kSortKeysThreads + threadIdx.x;
    uint32_t total;
    block_rank_of_kept(i < n && desc[i].pad == kFilterPass, wcnt, &total);
    if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kSortKeysThreads) void k_sort_keys(SortKeysArgs a, const uint64_t* __restrict__ group_base) {
    __shared__ uint32_t wcnt[kSortKeysThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kSortKeysThreads + threadIdx.x;
    const bool live = i < a.n;
    bool keep = live, bad = false;
    uint64_t key = 0, rec_off = 0;
    uint32_t len = 0;
    if (live) {
        const RecDesc d = a.desc[i];
        const int32_t ref = a.rec_ref[i];
        rec_off = d.rec_off;
        if (a.use_filter) { keep = d.pad == kFilterPass; bad = d.pad == kFilterBad; }
        else bad = ref < -1 || ref >= a.n_ref;
        if (keep && !bad) {
            const uint32_t bs = ld32(a.U + rec_off);                 // block_size
            len = bs + 4u;
            // (the chain of K2 ends every record inside the batch; a record that would not is never copied)
            bad = !record_len_ok(bs, rec_off, a.u_end);
            key = sortc::sort_key(ref, d.pos, d.flag, a.key_n_ref);
        }
        keep = keep && !bad;
    }
    const unsigned long long m = __ballot(keep);
    const unsigned long long mb = __ballot(bad);
    const uint32_t rank = block_rank_of_kept(keep, wcnt);
    const uint64_t gbase = group_base ? group_base[blockIdx.x] : (uint64_t)blockIdx.x * kSortKeysThreads;
    if (keep) {
        const uint64_t at = a.out_base + gbase + rank;
        a.key[at] = key;
        if (a.off) a.off[at] = (uint64_t)((int64_t)rec_off + a.store_delta);
        a.len[at] = len;
    }
    // the wave's share of the accumulators
    const unsigned long long k_or = wave_or(keep ? key : 0ull), k_and = wave_and(keep ? key : ~0ull), bytes = wave_sum<unsigned long long>(keep ? len : 0ull);
    if ((threadIdx.x & 63u) == 0) {
        if (m) {
            atomicOr(a.acc + kSortAccOr, k_or);
            atomicAnd(a.acc + kSortAccAnd, k_and);
            atomicAdd(a.acc + kSortAccKept, (unsigned long long)__popcll(m));
            atomicAdd(a.acc + kSortAccBytes, bytes);
        }
        if (mb) atomicAdd(a.acc + kSortAccBad, (unsigned long long)__popcll(mb));
    }
}

// ---- K9b -----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRadixThreads = 256, kRadixWaves = kRadixThreads / 64, kRadixRounds = kRadixTile / kRadixThreads;

__global__ __launch_bounds__(kRadixThreads) void k_radix_hist(const uint64_t* __restrict__ key, uint64_t n, uint32_t shift, uint32_t n_tiles,
                                                              uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * kRadixTile;
#pragma unroll 4
    for (uint32_t r = 0; r < kRadixRounds; ++r) {
        const uint64_t i = t0 + r * kRadixThreads + threadIdx.x;
        if (i < n) atomicAdd(&h[(uint32_t)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kRadixThreads) void k_radix_scatter(const uint64_t* __restrict__ key_in, const uint32_t* __restrict__ val_in,
                                                                 uint64_t* __restrict__ key_out, uint32_t* __restrict__ val_out, uint64_t n,
                                                                 uint32_t shift, uint32_t n_tiles, const uint64_t* __restrict__ hist_base) {
    __shared__ uint32_t off[256];                      // next output slot of every digit for this tile
    __shared__ uint32_t wcount[kRadixWaves][256];      // this round's elements per wave and digit
    const uint32_t t = threadIdx.x, wave = t >> 6;
    off[t] = (uint32_t)hist_base[(size_t)t * n_tiles + blockIdx.x];
#pragma unroll
    for (uint32_t w = 0; w < kRadixWaves; ++w) wcount[w][t] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * kRadixTile;
    const uint64_t lt = lanemask_lt();
    for (uint32_t r = 0; r < kRadixRounds; ++r) {
        const uint64_t i = t0 + r * kRadixThreads + t;
        if (t0 + r * kRadixThreads >= n) break;        // (workgroup-uniform)
        const bool live = i < n;
        uint64_t k = 0;
        uint32_t v = 0;
        if (live) { k = key_in[i]; v = val_in[i]; }
        const uint32_t digit = (uint32_t)(k >> shift) & 255u;
        // the live lanes of the wave that hold the same digit
        unsigned long long peers = __ballot(live);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const unsigned long long bal = __ballot(bit);
            peers &= bit ? bal : ~bal;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & lt);
        if (live && rank == 0) wcount[wave][digit] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (live) {
            uint32_t at = off[digit] + rank;
            for (uint32_t w = 0; w < wave; ++w) at += wcount[w][digit];
            key_out[at] = k;
            val_out[at] = v;
        }
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < kRadixWaves; ++w) { s += wcount[w][t]; wcount[w][t] = 0; }
        off[t] += s;
        __syncthreads();
    }
}

// ---- the pieces of the sorted stream (its offsets: launch_sorted_offsets, scan.hip) ------------------------------------------------
__global__ __launch_bounds__(256) void k_piece_bounds(const uint64_t* __restrict__ out_off, uint64_t n, uint64_t piece_bytes, uint32_t n_bounds,
                                                      uint32_t* __restrict__ rec) {
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_bounds) return;
    rec[k] = (uint32_t)sortc::first_record_ending_behind(out_off, n, (uint64_t)k * piece_bytes);
}

// ---- K9c -----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kGatherThreads = 256, kGatherRecs = kGatherThreads / kCopyGroup;

__global__ __launch_bounds__(kGatherThreads) void k_gather_records(const uint8_t* __restrict__ store, const uint64_t* __restrict__ off,
                                                                   const uint32_t* __restrict__ perm, const uint64_t* __restrict__ out_off,
                                                                   uint64_t r0, uint64_t r1, uint64_t p0, uint64_t p1, uint8_t* __restrict__ dst) {
    const uint64_t i = r0 + (uint64_t)blockIdx.x * kGatherRecs + threadIdx.x / kCopyGroup;
    if (i >= r1) return;
    sortc::PieceClip c;
    if (!sortc::clip_to_piece(out_off[i], out_off[i + 1], p0, p1, &c)) return;
    copy_span16(dst + c.dst, store + off[perm[i]] + c.src, c.len, threadIdx.x % kCopyGroup);
}

// ---- K9d -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_window_dest(const uint32_t* __restrict__ perm, const uint64_t* __restrict__ out_off, uint64_t n,
                                                     uint64_t* __restrict__ dest) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    const uint32_t i = perm[r];
    if (i < n) dest[i] = out_off[r];                    // (a permutation of [0, n): the test keeps the store inside dest whatever perm holds)
}

constexpr uint32_t kSpanThreads = 256;

__global__ __launch_bounds__(kSpanThreads) void k_batch_spans(const uint64_t* __restrict__ dest, const uint32_t* __restrict__ len,
                                                              const uint64_t* __restrict__ first, uint64_t* __restrict__ lo_out,
                                                              uint64_t* __restrict__ hi_out) {
    __shared__ uint64_t wlo[kSpanThreads / 64], whi[kSpanThreads / 64];
    const uint64_t i0 = first[blockIdx.x], i1 = first[blockIdx.x + 1];
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += kSpanThreads) {
        const uint64_t d = dest[i], e = d + len[i];
        lo = d < lo ? d : lo;
        hi = e > hi ? e : hi;
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if ((threadIdx.x & 63u) == 0) { wlo[threadIdx.x >> 6] = lo; whi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (uint32_t w = 1; w < kSpanThreads / 64; ++w) { lo = wlo[w] < lo ? wlo[w] : lo; hi = whi[w] > hi ? whi[w] : hi; }
        lo_out[blockIdx.x] = lo;
        hi_out[blockIdx.x] = hi;
    }
}

// the rank of every kept record among the kept records of the batch, as K9a numbers them (0xFFFFFFFF: not kept)
__global__ __launch_bounds__(kSortKeysThreads) void k_window_rank(const RecDesc* __restrict__ desc, uint64_t n, const uint64_t* __restrict__ group_base,
                                                                  uint32_t* __restrict__ rank_out) {
    __shared__ uint32_t wcnt[kSortKeysThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kSortKeysThreads + threadIdx.x;
    const bool keep = i < n && desc[i].pad == kFilterPass;
    const uint32_t rank = block_rank_of_kept(keep, wcnt);
    if (i < n) rank_out[i] = keep ? (uint32_t)group_base[blockIdx.x] + rank : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(kGatherThreads) void k_window_scatter(WindowScatterArgs a, const uint32_t* __restrict__ rank) {
    const uint64_t i = (uint64_t)blockIdx.x * kGatherRecs + threadIdx.x / kCopyGroup;
    const uint32_t l = threadIdx.x % kCopyGroup;
    bool bad = false;
    unsigned long long wrote = 0;
    if (i < a.n) {
        const uint64_t k = a.use_filter ? rank[i] : i;              // among the kept records of the batch
        if (!a.use_filter || k != 0xFFFFFFFFull) {
            const uint64_t rec_off = a.desc[i].rec_off;
            // the record as it is in THIS pass: its frame bounds the loads, the clip of [dest, dest + its length) the stores
            bad = k >= a.n_kept || rec_off + 4 > a.u_end;
            uint32_t bs = 0;
            if (!bad) { bs = ld32(a.U + rec_off); bad = !record_len_ok(bs, rec_off, a.u_end); }
            if (!bad) {
                const uint64_t ord = a.first_kept + k, len = (uint64_t)bs + 4u;
                bad = len != a.len[ord];
                sortc::PieceClip c;
                const uint64_t d = a.dest[ord];
                if (!bad && sortc::clip_to_piece(d, d + len, a.w0, a.w1, &c)) {
                    copy_span16(a.window + c.dst, a.U + rec_off + c.src, c.len, l);
                    wrote = l == 0 ? c.len : 0;
                }
            }
        }
    }
    const unsigned long long mb = __ballot(bad && l == 0);
    wrote = wave_sum(wrote);
    if ((threadIdx.x & 63u) == 0) {
        if (wrote) atomicAdd(a.acc + kWindowAccBytes, wrote);
        if (mb) atomicAdd(a.acc + kWindowAccMismatch, (unsigned long long)__popcll(mb));
    }
}

}  // namespace

void launch_window_dest(const uint32_t* d_perm, const uint64_t* d_out_off, uint64_t n, uint64_t* d_dest, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_window_dest, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_perm, d_out_off, n, d_dest);
    SBX_HIP(hipGetLastError());
}

void launch_batch_spans(const uint64_t* d_dest, const uint32_t* d_len, const uint64_t* d_first, uint32_t n_batches, uint64_t* d_lo,
                        uint64_t* d_hi, hipStream_t stream) {
    if (!n_batches) return;
    hipLaunchKernelGGL(k_batch_spans, dim3(n_batches), dim3(kSpanThreads), 0, stream, d_dest, d_len, d_first, d_lo, d_hi);
    SBX_HIP(hipGetLastError());
}

void launch_window_scatter(const WindowScatterArgs& a, uint32_t* d_group_count, uint64_t* d_group_base, uint32_t* d_rank, hipStream_t stream) {
    if (!a.n || a.w1 <= a.w0) return;
    if (a.use_filter) {
        const uint32_t groups = sort_keys_groups(a.n);
        hipLaunchKernelGGL(k_sort_group_count, dim3(groups), dim3(kSortKeysThreads), 0, stream, a.desc, a.n, d_group_count);
        SBX_HIP(hipGetLastError());
        launch_count_scan(d_group_count, groups, d_group_base, stream);
        hipLaunchKernelGGL(k_window_rank, dim3(groups), dim3(kSortKeysThreads), 0, stream, a.desc, a.n, d_group_base, d_rank);
        SBX_HIP(hipGetLastError());
    }
    const uint64_t groups = (a.n + kGatherRecs - 1) / kGatherRecs;
    hipLaunchKernelGGL(k_window_scatter, dim3((uint32_t)groups), dim3(kGatherThreads), 0, stream, a, a.use_filter ? d_rank : nullptr);
    SBX_HIP(hipGetLastError());
}

void launch_sort_keys(const SortKeysArgs& a, uint32_t* d_group_count, uint64_t* d_group_base, hipStream_t stream) {
    if (!a.n) return;
    const uint32_t groups = sort_keys_groups(a.n);
    if (a.use_filter) {
        hipLaunchKernelGGL(k_sort_group_count, dim3(groups), dim3(kSortKeysThreads), 0, stream, a.desc, a.n, d_group_count);
        SBX_HIP(hipGetLastError());
        launch_count_scan(d_group_count, groups, d_group_base, stream);
    }
    hipLaunchKernelGGL(k_sort_keys, dim3(groups), dim3(kSortKeysThreads), 0, stream, a, a.use_filter ? d_group_base : nullptr);
    SBX_HIP(hipGetLastError());
}

void launch_radix_pass(const uint64_t* d_key_in, const uint32_t* d_val_in, uint64_t* d_key_out, uint32_t* d_val_out, uint64_t n, uint32_t shift,
                       uint32_t* d_hist, uint64_t* d_hist_base, hipStream_t stream) {
    if (!n) return;
    const uint32_t tiles = radix_tiles(n);
    hipLaunchKernelGGL(k_radix_hist, dim3(tiles), dim3(kRadixThreads), 0, stream, d_key_in, n, shift, tiles, d_hist);
    SBX_HIP(hipGetLastError());
    launch_count_scan(d_hist, tiles * 256u, d_hist_base, stream);
    hipLaunchKernelGGL(k_radix_scatter, dim3(tiles), dim3(kRadixThreads), 0, stream, d_key_in, d_val_in, d_key_out, d_val_out, n, shift, tiles,
                       d_hist_base);
    SBX_HIP(hipGetLastError());
}

void launch_piece_bounds(const uint64_t* d_out_off, uint64_t n, uint64_t piece_bytes, uint32_t n_bounds, uint32_t* d_rec, hipStream_t stream) {
    if (!n_bounds) return;
    hipLaunchKernelGGL(k_piece_bounds, dim3((n_bounds + 255) / 256), dim3(256), 0, stream, d_out_off, n, piece_bytes, n_bounds, d_rec);
    SBX_HIP(hipGetLastError());
}

void launch_gather_records(const uint8_t* d_store, const uint64_t* d_off, const uint32_t* d_perm, const uint64_t* d_out_off, uint64_t r0,
                           uint64_t r1, uint64_t p0, uint64_t p1, uint8_t* d_dst, hipStream_t stream) {
    if (r1 <= r0 || p1 <= p0) return;
    const uint64_t groups = (r1 - r0 + kGatherRecs - 1) / kGatherRecs;
    hipLaunchKernelGGL(k_gather_records, dim3((uint32_t)groups), dim3(kGatherThreads), 0, stream, d_store, d_off, d_perm, d_out_off, r0, r1, p0, p1,
                       d_dst);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
