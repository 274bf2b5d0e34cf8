// view.hip -- K12: the record selection of `sambamba view` (sambamba/view.d) on the records K2 described.
//
//   K12a k_view_select   one lane per described record of a batch: K2's filter verdict (RecDesc::pad), --num-filter on RecDesc::flag,
//                        -s (64-bit FNV-1a over the name bytes in U, single-byte loads at any address, then the seed) and the region
//                        part over RecDesc::pos / end: for merged regions (-L; disjoint, sorted by (ref, start)) a binary search for
//                        the first region that ends behind pos -- the only one the record can overlap first --, for listed regions a
//                        loop over the list (wave-uniform addresses) that counts the regions the record overlaps.  The lane's
//                        number of entries (0, 1, or one per overlapped region) is stored; the entries and the selected records of a
//                        workgroup are summed (block_sum, block_rank_of_kept: wave_prims.hpp) so that two exclusive scans
//                        (launch_count_scan) give every workgroup its first output slots -- the file-order-preserving compaction
//                        of K9a.  For -c nothing is stored: one atomicAdd per wave into the file's counter.  With -v the lane first
//                        reads the mask K19 left for its record (ViewSelectArgs::invalid): not 0, and nothing else is asked.
//   K12b k_view_emit     the same lanes again: a selected record's ordinal is the workgroup's base + the selected threads in front
//                        of it (block_rank_of_kept), its first entry the base + an exclusive prefix of the counts (block_exclusive).
//                        Store offset and length are written once per record; for listed regions the list is walked again and
//                        (region index, record ordinal) written per overlapped region, in listed order.
//   k_view_compose       perm[i] = entry_rec[order[i]]: the sorted entries (K9b over the region index) as record ordinals, the form
//                        plan_output / K9c read.
//   K12c k_view_order    the indexed view only: one lane per described record, its (ref_id, pos) against the record in front of it
//                        (the batch before for lane 0: a key the host carries over); one coalesced read of RecDesc and rec_ref
//                        per record and of the neighbour's, which the cache holds; a wave that saw a decrease ORs 1 into the flag.
//
// Bytes moved (n records of a batch, s of them selected, e entries, r listed regions): K12a reads 36 n (descriptor, rec_ref), with -s
// the name bytes (scattered, <= 254 each), with BAM output 4 s scattered words of U, and 12 r per wave through the scalar cache;
// it writes 4 n + 8 n / 256.  K12b reads 40 n + 4 s of U and writes 12 s + 12 e.  -c writes nothing but one atomic per wave.
#include "common.hpp"
#include "view.hpp"
#include "view_core.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// is the record (ref, pos, covered) in the merged list?  g = the first region, in (ref, start) order, with (ref, end) > (ref, pos):
// every region in front of it ends at or before pos, every region behind it starts later than g does.
__device__ __forceinline__ bool in_merged(const sbx_region* __restrict__ regs, uint32_t n, int32_t ref, int32_t pos, uint32_t covered) {
    if (ref < 0) return false;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const sbx_region g = regs[mid];
        const bool behind = g.ref_id > (uint32_t)ref || (g.ref_id == (uint32_t)ref && (int64_t)g.end > (int64_t)pos);
        if (behind) hi = mid; else lo = mid + 1;
    }
    if (lo >= n) return false;
    const sbx_region g = regs[lo];
    return viewc::overlaps(ref, pos, covered, g.ref_id, g.start, g.end);
}

// everything but the region part; *bad: the record is malformed
__device__ __forceinline__ bool passes_filters(const ViewSelectArgs& a, const RecDesc& d, bool* bad) {
    *bad = d.pad == kFilterBad;
    if (d.pad != kFilterPass) return false;
    if (!viewc::flags_pass(d.flag, a.flags_set, a.flags_unset)) return false;
    if (a.subsample) {
        const uint32_t name_len = d.l_name ? d.l_name - 1u : 0u;
        if (d.rec_off + 36ull + name_len > a.u_end) { *bad = true; return false; }
        if (!viewc::subsample_keeps(viewc::name_seed_hash(a.U + d.rec_off + 36, name_len, a.seed), a.threshold)) return false;
    }
    return true;
}

__global__ __launch_bounds__(kViewThreads) void k_view_select(ViewSelectArgs a) {
    __shared__ uint32_t w_entries[kViewThreads / 64], w_records[kViewThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kViewThreads + threadIdx.x;
    uint32_t cnt = 0;
    bool bad = false;
    int32_t ref = -1, pos = 0;
    uint32_t covered = 0;
    uint64_t rec_off = 0;
    bool pass = false;
    if (i < a.n) {
        const RecDesc d = a.desc[i];
        ref = a.rec_ref[i];
        pos = d.pos;
        covered = (uint32_t)(d.end - d.pos);
        rec_off = d.rec_off;
        pass = !(a.invalid && a.invalid[i]) && passes_filters(a, d, &bad);
    }
    if (a.n_regions == 0) cnt = pass ? 1u : 0u;
    else if (a.regions_merged) cnt = pass && in_merged(a.regions, a.n_regions, ref, pos, covered) ? 1u : 0u;
    else {
        for (uint32_t r = 0; r < a.n_regions; ++r) {          // (the address is the same in every lane)
            const sbx_region g = a.regions[r];
            cnt += pass && viewc::overlaps(ref, pos, covered, g.ref_id, g.start, g.end) ? 1u : 0u;
        }
    }
    uint32_t len = 0;
    if (cnt && a.with_lengths) {
        const uint32_t bs = ld32(a.U + rec_off);              // block_size
        len = bs + 4u;
        if (!record_len_ok(bs, rec_off, a.u_end)) { bad = true; cnt = 0; len = 0; }
    }
    if (a.count && i < a.n) a.count[i] = cnt;
    // the wave's share
    const unsigned long long entries = wave_sum<unsigned long long>(cnt), bytes = wave_sum((unsigned long long)cnt * len);
    const unsigned long long m = __ballot(cnt != 0), mb = __ballot(bad);
    if ((threadIdx.x & 63u) == 0) {
        if (m) {
            atomicAdd(a.acc + kViewAccEntries, entries);
            atomicAdd(a.acc + kViewAccRecords, (unsigned long long)__popcll(m));
            if (bytes) atomicAdd(a.acc + kViewAccBytes, bytes);
        }
        if (mb) atomicAdd(a.acc + kViewAccBad, (unsigned long long)__popcll(mb));
    }
    if (!a.group_entries) return;                              // (uniform: -c)
    // the workgroup's share: what the two scans of the host turn into the first output slots of K12b
    uint32_t records;
    block_rank_of_kept(cnt != 0, w_records, &records);
    const uint32_t all = block_sum(cnt, w_entries);
    if (threadIdx.x == 0) {
        a.group_entries[blockIdx.x] = all;
        a.group_records[blockIdx.x] = records;
    }
}

__global__ __launch_bounds__(kViewThreads) void k_view_emit(ViewEmitArgs a) {
    __shared__ uint32_t w_entries[kViewThreads / 64], w_records[kViewThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kViewThreads + threadIdx.x;
    const uint32_t cnt = i < a.s.n ? a.s.count[i] : 0u;
    // the selected records and the entries of the threads in front, inside the workgroup
    uint32_t all;
    const uint32_t e_before = block_exclusive(cnt, w_entries, &all);
    const uint32_t r_before = block_rank_of_kept(cnt != 0, w_records);
    if (!cnt) return;
    const RecDesc d = a.s.desc[i];
    const uint64_t ord = a.record_base + a.group_record_base[blockIdx.x] + r_before;
    a.off[ord] = (uint64_t)((int64_t)d.rec_off + a.store_delta);
    a.len[ord] = ld32(a.s.U + d.rec_off) + 4u;                 // (checked by K12a: a record that fails has no entries)
    if (!a.entry_key) return;
    uint64_t at = a.entry_base + a.group_entry_base[blockIdx.x] + e_before;
    const int32_t ref = a.s.rec_ref[i];
    const uint32_t covered = (uint32_t)(d.end - d.pos);
    uint32_t left = cnt;
    for (uint32_t r = 0; r < a.s.n_regions && left; ++r) {
        const sbx_region g = a.s.regions[r];
        if (viewc::overlaps(ref, d.pos, covered, g.ref_id, g.start, g.end)) {
            a.entry_key[at] = r;
            a.entry_rec[at] = (uint32_t)ord;
            ++at;
            --left;
        }
    }
}

__global__ __launch_bounds__(256) void k_view_compose(const uint32_t* __restrict__ entry_rec, const uint32_t* __restrict__ order, uint64_t n,
                                                      uint32_t* __restrict__ perm) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) perm[i] = entry_rec[order[i]];
}

__device__ __forceinline__ uint64_t order_key(int32_t ref, int32_t pos) {
    return ref < 0 ? 0ull : ((uint64_t)((uint32_t)ref + 1u) << 32) | (uint32_t)(pos + 1);
}

__global__ __launch_bounds__(kViewThreads) void k_view_order(const RecDesc* __restrict__ desc, const int32_t* __restrict__ rec_ref, uint64_t n,
                                                            uint64_t prev_key, uint32_t* __restrict__ unsorted,
                                                            unsigned long long* __restrict__ last_key) {
    const uint64_t i = (uint64_t)blockIdx.x * kViewThreads + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const uint64_t key = order_key(rec_ref[i], desc[i].pos);
        const uint64_t before = i ? order_key(rec_ref[i - 1], desc[i - 1].pos) : prev_key;
        bad = key != 0 && before != 0 && key < before;
        if (i + 1 == n) *last_key = key;
    }
    if (__ballot(bad) && (threadIdx.x & 63u) == 0) atomicOr(unsorted, 1u);
}

}  // namespace

void launch_view_order(const RecDesc* d_desc, const int32_t* d_rec_ref, uint64_t n, uint64_t prev_key, uint32_t* d_unsorted,
                       unsigned long long* d_last_key, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_view_order, dim3(view_groups(n)), dim3(kViewThreads), 0, stream, d_desc, d_rec_ref, n, prev_key, d_unsorted, d_last_key);
    SBX_HIP(hipGetLastError());
}

void launch_view_select(const ViewSelectArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_view_select, dim3(view_groups(a.n)), dim3(kViewThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_view_emit(const ViewEmitArgs& a, hipStream_t stream) {
    if (!a.s.n) return;
    hipLaunchKernelGGL(k_view_emit, dim3(view_groups(a.s.n)), dim3(kViewThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_view_compose(const uint32_t* d_entry_rec, const uint32_t* d_order, uint64_t n, uint32_t* d_perm, hipStream_t stream) {
    if (!n) return;
    hipLaunchKernelGGL(k_view_compose, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, d_entry_rec, d_order, n, d_perm);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
