// merge.hip -- K11: the device side of `sambamba merge` (sambamba/merge.d:133-207, `modifier`): the records of one read batch of one
// input are rewritten on their way into the resident record store.
//
//   K11a k_merge_describe  one lane per described record.  Every length the record states is checked against its block_size and the
//                          batch before a byte behind the fixed part is read (read_record_frame, wave_prims.hpp, as in K10a; the
//                          reference ids are those of the input's own dictionary); then the aux fields are walked, every
//                          type's size checked against the record end -- `B` arrays by element type and count, `Z` / `H` to a NUL
//                          inside the record.  The value of the first RG:Z and of the first PG:Z field is looked up in the input's
//                          rename table (only the ids that change, compared byte for byte); a hit is a patch: offset of the old
//                          value, table entry.  Out come the new record length, up to two patches, and the sort key
//                          (sort_core.hpp) of the REWRITTEN record: merged reference id, merged number of references.  A record
//                          that fails a check is counted and the call ends with SBX_EFORMAT.  With -F the verdict K2 left in
//                          RecDesc::pad decides, on the record as it is in its input.
//   scans                  launch_sorted_offsets (scan.hip) over the new lengths and over the keep flags: where a record starts
//                          behind the store's fill, and its record number behind the records kept before.
//   K11b k_merge_rewrite   sixteen lanes per record (K9c's partition).  The first 36 bytes go out byte by byte with block_size,
//                          ref_id and next_ref_id replaced (-1 stays -1; a next_ref_id outside the input's dictionary stays as it
//                          is); the stretches between the patches move as K9c moves a record (copy_span16, wave_prims.hpp); the
//                          new ids are written byte by byte.  Plain C++ vector stores.  The host has compared the scanned size of
//                          the batch with what is left of the store before the launch: no lane writes behind store_at + len_base[n].
//        k_merge_emit_keys the key pass of the windowed merge (launch_merge_rewrite without a store): one lane per record, key and
//                          NEW length to the record's ordinal, no byte moved.
//   K11c k_merge_window_scatter  the windowed merge (engine_merge.cpp: inputs that do not stay on the device): sixteen lanes per
//                          described record of a REPLAYED batch that K11a has described again, the shape of K11b and of K9d-3
//                          (sort.hip).  The record's ordinal is the batch's saved first ordinal + keep_base[i], its place in the
//                          merged stream dest[ordinal]; the stretches K11b writes -- fixed part, source, new id, source, new id,
//                          tail -- are each clipped to the window [w0, w1) (mergewin_core.hpp: for_each_stretch) and go to
//                          window + (dest - w0): source stretches with copy_span16, the fixed part and the ids byte by byte.  The
//                          clip is what bounds the stores; the frame K11a checked in THIS pass bounds the loads.  Every wave adds
//                          the bytes it wrote to one 64-bit counter and the records that are not the ones of the key pass (another
//                          new length; a batch that keeps another number of records) to a second (sort.hpp WindowAcc).
//
// Bytes moved (n records, b bytes): K11a reads 32 n of descriptors and the fixed part + aux fields of every record, writes 36 n;
// the scans read and write 24 n; K11b reads and writes b; the emit reads 24 n and writes 12 n.  K11c, for a window of w bytes filled
// from batches of r records: K11a and the scans over the r records again, then 48 r (keep, keep_base, new_len, saved length, dest,
// descriptor, patches) + w read and w written.
#include "common.hpp"
#include "merge.hpp"
#include "mergewin_core.hpp"
#include "sort_core.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// the entry of `kind` whose old id is the n bytes at v; kMergeNone: the id does not change.  A linear scan, one lane per record,
// byte loads: written for the handful of colliding ids of per-lane files (a table of a few entries, which stays in cache).  The
// cost is O(records x table); an input with hundreds of renamed ids wants the table sorted by (kind, length, bytes) and a binary
// search here.  Not measured.
__device__ uint32_t find_rename(const RenameTable& t, uint32_t kind, const uint8_t* v, uint32_t n) {
    for (uint32_t e = 0; e < t.n; ++e) {
        const RenameEntry x = t.entry[e];
        if (x.kind != kind || x.old_len != n) continue;
        uint32_t k = 0;
        while (k < n && (uint8_t)t.blob[x.old_off + k] == v[k]) ++k;
        if (k == n) return e;
    }
    return kMergeNone;
}

__device__ __forceinline__ int32_t map_ref(const MergeArgs& a, int32_t ref) { return ref >= 0 && ref < a.n_ref_own ? a.ref_map[ref] : ref; }

// ---- K11a ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMergeThreads) void k_merge_describe(MergeArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
    const bool live = i < a.n;
    bool keep = live, bad = false, changed = false;
    uint32_t old_len = 0, new_len = 0;
    uint32_t pat[2] = {0u, 0u}, pen[2] = {kMergeNone, kMergeNone};
    uint64_t key = 0;
    if (live) {
        const RecDesc d = a.desc[i];
        const uint64_t rec_off = d.rec_off;
        if (a.use_filter) { keep = d.pad == kFilterPass; bad = d.pad == kFilterBad; }
        if (keep && !bad) {
            const uint8_t* p = a.U + rec_off;
            RecordFrame f;
            bad = !read_record_frame(a.U, rec_off, a.u_end, a.n_ref_own, &f);
            if (!bad) {
                old_len = f.bs + 4u;
                int64_t grow = 0;
                uint32_t np = 0;
                bool seen[2] = {false, false};
                uint64_t t = 4 + f.fixed;
                const uint64_t e = 4ull + f.bs;
                while (t < e) {
                    if (t + 3 > e) { bad = true; break; }
                    const uint8_t k0 = p[t], k1 = p[t + 1], ty = p[t + 2];
                    t += 3;
                    const uint64_t v = t;
                    switch (ty) {
                        case 'A': case 'c': case 'C': t += 1; break;
                        case 's': case 'S': t += 2; break;
                        case 'i': case 'I': case 'f': t += 4; break;
                        case 'Z': case 'H':
                            while (t < e && p[t]) ++t;
                            ++t;                                   // (t > e now: no NUL inside the record)
                            break;
                        case 'B': {
                            if (t + 5 > e) { t = e + 1; break; }
                            const uint8_t sub = p[t];
                            const uint32_t cnt = ld32(p + t + 1);
                            uint32_t w = 0;
                            if (sub == 'c' || sub == 'C') w = 1; else if (sub == 's' || sub == 'S') w = 2; else if (sub == 'i' || sub == 'I' || sub == 'f') w = 4;
                            t = w ? t + 5 + (uint64_t)cnt * w : e + 1;
                            break;
                        }
                        default: t = e + 1; break;
                    }
                    if (t > e) { bad = true; break; }
                    if (ty != 'Z') continue;
                    const uint32_t kind = (k0 == 'R' && k1 == 'G') ? 0u : (k0 == 'P' && k1 == 'G') ? 1u : 2u;
                    if (kind == 2u || seen[kind]) continue;
                    seen[kind] = true;
                    const uint32_t en = a.table.n ? find_rename(a.table, kind, p + v, (uint32_t)(t - 1 - v)) : kMergeNone;
                    if (en != kMergeNone) {
                        pat[np] = (uint32_t)v;
                        pen[np] = en;
                        ++np;
                        grow += (int64_t)a.table.entry[en].new_len - (int64_t)a.table.entry[en].old_len;
                    }
                }
                if (!bad) {
                    const int64_t nl = (int64_t)old_len + grow;
                    bad = nl < 36 || nl > 0x7FFFFFF0ll;
                    new_len = (uint32_t)nl;
                    const int32_t new_ref = map_ref(a, f.ref), new_next = map_ref(a, f.next_ref);
                    changed = np != 0 || new_ref != f.ref || new_next != f.next_ref;
                    key = sortc::sort_key(new_ref, f.pos, f.flag, a.n_ref_merged);
                }
            }
        }
        keep = keep && !bad;
        if (!keep) { new_len = 0; old_len = 0; changed = false; }
        a.b.new_len[i] = new_len;
        a.b.keep[i] = keep ? 1u : 0u;
        a.b.key[i] = key;
        a.b.patch_at[2 * i] = pat[0]; a.b.patch_at[2 * i + 1] = pat[1];
        a.b.patch_entry[2 * i] = keep ? pen[0] : kMergeNone; a.b.patch_entry[2 * i + 1] = keep ? pen[1] : kMergeNone;
    }
    // the wave's share of the accumulators
    const unsigned long long m = __ballot(keep), mb = __ballot(bad), mc = __ballot(changed);
    const unsigned long long k_or = wave_or(keep ? key : 0ull), k_and = wave_and(keep ? key : ~0ull);
    const unsigned long long bytes = wave_sum<unsigned long long>(new_len), old_bytes = wave_sum<unsigned long long>(old_len);
    if ((threadIdx.x & 63u) == 0) {
        if (m) {
            atomicOr(a.acc + kSortAccOr, k_or);
            atomicAnd(a.acc + kSortAccAnd, k_and);
            atomicAdd(a.acc + kSortAccKept, (unsigned long long)__popcll(m));
            atomicAdd(a.acc + kSortAccBytes, bytes);
            atomicAdd(a.acc + kMergeAccOldBytes, old_bytes);
        }
        if (mc) atomicAdd(a.acc + kMergeAccRewritten, (unsigned long long)__popcll(mc));
        if (mb) atomicAdd(a.acc + kSortAccBad, (unsigned long long)__popcll(mb));
    }
}

// ---- K11b ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kRewriteGroup = kCopyGroup, kRewriteRecs = kMergeThreads / kRewriteGroup;

__global__ __launch_bounds__(kMergeThreads) void k_merge_rewrite(MergeArgs a) {
    const uint32_t l = threadIdx.x % kRewriteGroup;
    const uint64_t i = (uint64_t)blockIdx.x * kRewriteRecs + threadIdx.x / kRewriteGroup;
    if (i >= a.n || !a.b.keep[i]) return;
    const uint32_t nl = a.b.new_len[i];
    const uint64_t at = a.store_at + a.b.len_base[i];
    const uint8_t* src = a.U + a.desc[i].rec_off;
    uint8_t* dst = a.store + at;
    const uint32_t old_len = ld32(src) + 4u;
    // the fixed part up to the read name, with the three words that change
    const uint32_t new_ref = (uint32_t)map_ref(a, (int32_t)ld32(src + 4)), new_next = (uint32_t)map_ref(a, (int32_t)ld32(src + 24));
    for (uint32_t b = l; b < 36u; b += kRewriteGroup) {
        const uint32_t w = b >> 2;
        const uint32_t v = w == 0 ? nl - 4u : w == 1 ? new_ref : w == 6 ? new_next : ld32(src + 4 * w);
        dst[b] = (uint8_t)(v >> (8 * (b & 3u)));
    }
    uint64_t s_pos = 36, d_pos = 36;
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t en = a.b.patch_entry[2 * i + k];
        if (en == kMergeNone) break;
        const uint32_t p_at = a.b.patch_at[2 * i + k];
        const RenameEntry x = a.table.entry[en];
        copy_span16(dst + d_pos, src + s_pos, p_at - s_pos, l);
        d_pos += p_at - s_pos;
        for (uint32_t b = l; b < x.new_len; b += kRewriteGroup) dst[d_pos + b] = (uint8_t)a.table.blob[x.new_off + b];
        d_pos += x.new_len;
        s_pos = (uint64_t)p_at + x.old_len;
    }
    copy_span16(dst + d_pos, src + s_pos, old_len - s_pos, l);
    if (l == 0) {
        const uint64_t r = a.out_base + a.b.keep_base[i];
        a.key[r] = a.b.key[i];
        a.off[r] = at;
        a.len[r] = nl;
    }
}

// the key pass of the windowed merge: what K11b's lane 0 writes, without the bytes and without an offset
__global__ __launch_bounds__(kMergeThreads) void k_merge_emit_keys(MergeArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kMergeThreads + threadIdx.x;
    if (i >= a.n || !a.b.keep[i]) return;
    const uint64_t r = a.out_base + a.b.keep_base[i];
    a.key[r] = a.b.key[i];
    a.len[r] = a.b.new_len[i];
}

// ---- K11c ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMergeThreads) void k_merge_window_scatter(MergeArgs a, MergeWindowArgs w) {
    const uint32_t l = threadIdx.x % kRewriteGroup;
    const uint64_t i = (uint64_t)blockIdx.x * kRewriteRecs + threadIdx.x / kRewriteGroup;
    bool bad = false;
    unsigned long long wrote = 0;
    if (i < a.n && a.b.keep[i]) {
        const uint64_t k = a.b.keep_base[i];                       // among the records of the batch that take part
        bad = a.b.keep_base[a.n] != w.n_kept || k >= w.n_kept;
        if (!bad) {
            const uint64_t ord = w.first_kept + k;
            const uint32_t nl = a.b.new_len[i];
            bad = nl != w.len[ord];
            const uint64_t d = w.dest[ord];
            if (!bad && d < w.w1 && d + nl > w.w0) {
                // the record as K11a found it in THIS pass: its frame and its patches bound the loads, the clips the stores
                const uint8_t* src = a.U + a.desc[i].rec_off;
                const uint32_t old_len = ld32(src) + 4u;
                const uint32_t new_ref = (uint32_t)map_ref(a, (int32_t)ld32(src + 4)), new_next = (uint32_t)map_ref(a, (int32_t)ld32(src + 24));
                mergewin::Patch patch[mergewin::kMaxPatches];
                uint32_t np = 0;
                for (uint32_t q = 0; q < mergewin::kMaxPatches; ++q) {
                    const uint32_t en = a.b.patch_entry[2 * i + q];
                    if (en == kMergeNone) break;
                    const RenameEntry x = a.table.entry[en];
                    patch[np++] = mergewin::Patch{a.b.patch_at[2 * i + q], x.old_len, x.new_len, x.new_off};
                }
                mergewin::for_each_stretch(old_len, nl, patch, np, d, w.w0, w.w1, [&](uint32_t kind, uint64_t s, uint64_t at, uint64_t len) {
                    uint8_t* out = w.window + at;
                    if (kind == mergewin::kStretchSource) {
                        copy_span16(out, src + s, len, l);
                    } else if (kind == mergewin::kStretchBlob) {
                        for (uint64_t b = l; b < len; b += kRewriteGroup) out[b] = (uint8_t)a.table.blob[s + b];
                    } else {
                        for (uint64_t b = l; b < len; b += kRewriteGroup) {
                            const uint32_t fb = (uint32_t)(s + b);
                            out[b] = mergewin::fixed_byte(fb, nl - 4u, new_ref, new_next, ld32(src + 4 * (fb >> 2)));
                        }
                    }
                    wrote += len;
                });
                if (l != 0) wrote = 0;
            }
        }
    }
    const unsigned long long mb = __ballot(bad && l == 0);
    wrote = wave_sum(wrote);
    if ((threadIdx.x & 63u) == 0) {
        if (wrote) atomicAdd(w.acc + kWindowAccBytes, wrote);
        if (mb) atomicAdd(w.acc + kWindowAccMismatch, (unsigned long long)__popcll(mb));
    }
}

}  // namespace

void launch_merge_describe(const MergeArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_merge_describe, dim3((uint32_t)((a.n + kMergeThreads - 1) / kMergeThreads)), dim3(kMergeThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
    launch_sorted_offsets(a.b.new_len, nullptr, a.n, 0, a.b.tile_sum, a.b.len_base, stream);
    launch_sorted_offsets(a.b.keep, nullptr, a.n, 0, a.b.tile_sum, a.b.keep_base, stream);
}

void launch_merge_rewrite(const MergeArgs& a, hipStream_t stream) {
    if (!a.n) return;
    if (!a.store) {
        hipLaunchKernelGGL(k_merge_emit_keys, dim3((uint32_t)((a.n + kMergeThreads - 1) / kMergeThreads)), dim3(kMergeThreads), 0, stream, a);
        SBX_HIP(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL(k_merge_rewrite, dim3((uint32_t)((a.n + kRewriteRecs - 1) / kRewriteRecs)), dim3(kMergeThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_merge_window_scatter(const MergeArgs& a, const MergeWindowArgs& w, hipStream_t stream) {
    if (!a.n || w.w1 <= w.w0) return;
    hipLaunchKernelGGL(k_merge_window_scatter, dim3((uint32_t)((a.n + kRewriteRecs - 1) / kRewriteRecs)), dim3(kMergeThreads), 0, stream, a, w);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
