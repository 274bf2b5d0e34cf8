// slice.hip -- K18: the edge logic of `sambamba slice` (sambamba/slice.d) on the records K2 described in the edge runs of a call.
//
//   K18a k_slice_select  one lane per described record, all regions of the call at once.  Two binary searches over the sorted edge
//                        positions: the last edge (ref, x) at or in front of the record's (ref, pos) -- the record is a candidate for
//                        first_ge of that edge and, the file being sorted, of every edge of the contig in front of it; the first lane
//                        of a run of equal edges in the wave (it has the lowest offset) sends one 64-bit atomicMin, and the host takes
//                        the suffix minimum over the edges of a contig.  Two more over the region starts give the regions whose beg
//                        lies in (pos, pos + covered): their R1 holds the record (slicec::in_r1 confirms each).  The lane's number of
//                        entries is stored, per region count and bytes are added up, and the entries of a workgroup are summed
//                        (block_sum, wave_prims.hpp) for the exclusive scan that keeps the compaction in file order.
//   K18b k_slice_emit    the same lanes again: (4 * region, rec_off, length) per entry at the workgroup's base + an exclusive prefix of
//                        the counts (block_exclusive).  The stable sort of the keys (K9b) then orders them by region.
//
// Work is assigned by record, not by region: a BED file of hundreds of thousands of regions costs four binary searches per record.
// Bytes moved (n records, e entries): K18a reads 36 n + 4 e scattered words of U and writes 4 n + 4 n / 256 + its atomics; K18b
// reads 40 n and writes 20 e.  Both are bound by the latency of the dependent loads of the searches, not by bandwidth.
#include "common.hpp"
#include "slice.hpp"
#include "slice_core.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// the first edge / region start, in (ref, x) order, that lies behind (or, with `or_equal`, at or behind) (ref, p)
template <class T, class X>
__device__ __forceinline__ uint32_t first_behind(const T* __restrict__ v, uint32_t n, X x_of, uint32_t ref, int64_t p, bool or_equal) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const T g = v[mid];
        const int64_t x = (int64_t)x_of(g);
        const bool behind = g.ref_id > ref || (g.ref_id == ref && (or_equal ? x >= p : x > p));
        if (behind) hi = mid; else lo = mid + 1;
    }
    return lo;
}

struct Lane {
    uint32_t cnt, lo, hi, len;
    bool bad;
};

// the R1 part of record i: the region starts [lo, hi) it may belong to and how many of them it does
__device__ __forceinline__ Lane r1_of(const SliceSelectArgs& a, const RecDesc& d, int32_t ref) {
    Lane l{0u, 0u, 0u, 0u, d.pad == kFilterBad};
    if (l.bad || ref < 0 || d.end <= d.pos) return l;
    auto beg_of = [](const SliceBeg& g) { return g.beg; };
    l.lo = first_behind(a.begs, a.n_begs, beg_of, (uint32_t)ref, (int64_t)d.pos, false);
    l.hi = first_behind(a.begs, a.n_begs, beg_of, (uint32_t)ref, (int64_t)d.end, true);
    const uint32_t covered = (uint32_t)(d.end - d.pos);
    for (uint32_t j = l.lo; j < l.hi; ++j) {
        const SliceBeg g = a.begs[j];
        l.cnt += slicec::in_r1(ref, d.pos, covered, g.ref_id, g.beg) ? 1u : 0u;
    }
    return l;
}

__global__ __launch_bounds__(kSliceThreads) void k_slice_select(SliceSelectArgs a) {
    __shared__ uint32_t w_entries[kSliceThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kSliceThreads + threadIdx.x;
    Lane l{0u, 0u, 0u, 0u, false};
    uint32_t slot = 0xFFFFFFFFu;
    uint64_t rec_off = 0;
    int32_t ref = -1;
    RecDesc d{};
    if (i < a.n) {
        d = a.desc[i];
        ref = a.rec_ref[i];
        rec_off = d.rec_off;
        l = r1_of(a, d, ref);
        if (!l.bad && ref >= 0 && a.n_edges) {
            // the last edge at or in front of (ref, pos)
            const uint32_t k = first_behind(a.edges, a.n_edges, [](const SliceEdge& e) { return e.x; }, (uint32_t)ref, (int64_t)d.pos, false);
            if (k > 0) {
                const SliceEdge e = a.edges[k - 1];
                if (e.ref_id == (uint32_t)ref && slicec::at_or_behind(ref, d.pos, e.ref_id, e.x)) slot = k - 1;
            }
        }
        if (l.cnt) {
            const uint32_t bs = ld32(a.U + rec_off);
            l.len = bs + 4u;
            if (!record_len_ok(bs, rec_off, a.u_end)) { l.bad = true; l.cnt = 0; l.len = 0; }
        }
        a.count[i] = l.cnt;
    }
    // first_ge: one atomic per run of equal edges in the wave; offsets grow with the lane, so its first lane holds the minimum
    const uint32_t prev = __shfl_up(slot, 1, 64);
    if (slot != 0xFFFFFFFFu && ((threadIdx.x & 63u) == 0 || prev != slot)) atomicMin(a.edge_min + slot, (unsigned long long)rec_off);
    // R1: per region
    if (l.cnt) {
        const uint32_t covered = (uint32_t)(d.end - d.pos);
        for (uint32_t j = l.lo; j < l.hi; ++j) {
            const SliceBeg g = a.begs[j];
            if (!slicec::in_r1(ref, d.pos, covered, g.ref_id, g.beg)) continue;
            atomicAdd(a.region_count + g.region, 1u);
            atomicAdd(a.region_bytes + g.region, (unsigned long long)l.len);
        }
    }
    const unsigned long long entries = wave_sum<unsigned long long>(l.cnt), bytes = wave_sum((unsigned long long)l.cnt * l.len);
    const unsigned long long mb = __ballot(l.bad);
    if ((threadIdx.x & 63u) == 0) {
        if (entries) {
            atomicAdd(a.acc + kSliceAccEntries, entries);
            atomicAdd(a.acc + kSliceAccBytes, bytes);
        }
        if (mb) atomicAdd(a.acc + kSliceAccBad, (unsigned long long)__popcll(mb));
    }
    const uint32_t all = block_sum(l.cnt, w_entries);
    if (threadIdx.x == 0) a.group_entries[blockIdx.x] = all;
}

__global__ __launch_bounds__(kSliceThreads) void k_slice_emit(SliceEmitArgs a) {
    __shared__ uint32_t w_entries[kSliceThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kSliceThreads + threadIdx.x;
    const uint32_t cnt = i < a.s.n ? a.s.count[i] : 0u;
    uint32_t all;
    const uint32_t e_before = block_exclusive(cnt, w_entries, &all);
    if (!cnt) return;
    const RecDesc d = a.s.desc[i];
    const int32_t ref = a.s.rec_ref[i];
    const Lane l = r1_of(a.s, d, ref);
    const uint32_t len = ld32(a.s.U + d.rec_off) + 4u;             // (checked by K18a: a record that fails has no entries)
    const uint32_t covered = (uint32_t)(d.end - d.pos);
    uint64_t at = a.group_entry_base[blockIdx.x] + e_before;
    uint32_t left = cnt;
    for (uint32_t j = l.lo; j < l.hi && left; ++j) {
        const SliceBeg g = a.s.begs[j];
        if (!slicec::in_r1(ref, d.pos, covered, g.ref_id, g.beg)) continue;
        a.key[at] = 4ull * g.region;
        a.off[at] = d.rec_off;
        a.len[at] = len;
        ++at;
        --left;
    }
}

}  // namespace

void launch_slice_select(const SliceSelectArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_slice_select, dim3(slice_groups(a.n)), dim3(kSliceThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_slice_emit(const SliceEmitArgs& a, hipStream_t stream) {
    if (!a.s.n) return;
    hipLaunchKernelGGL(k_slice_emit, dim3(slice_groups(a.s.n)), dim3(kSliceThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
