// stream.hip -- K21: the selected records of one described batch into a staging window of the output stream, for the commands whose
// output order is the input order (view with the BAM sink, fixbins) when the file is written without a record store
// (engine_streamout.hpp).  The batch is still in U; every selected byte is read once from there and written once into the window.
//
//   K21a k_pack_lengths  one lane per described record: the verdict of K12a (null: every record), the record's length (block_size + 4,
//                        read from U at any byte address; 0 when the frame does not lie inside the batch), stored; the lengths of a
//                        workgroup are added up in 64 bits (block_sum).  launch_scan64 over the group sums gives every workgroup its
//                        base.
//   K21b                 launch_group_offsets (scan.hip), the kernel K13a's line offsets use: dest[i] = the batch's place in the
//                        stream + the group's base + the lengths in front of i inside its group.  K21a and K21b run once per batch;
//                        the price of deriving dest once per batch and not once per window is that K21c reads dest and len again,
//                        12 n bytes, for every window the batch meets.
//   K21c k_pack_records  sixteen lanes per record, the shape of K9c and K9d-3: the record's bytes, clipped to the window [w0, w1)
//                        (streamc::plan_record), go from U to window + (dest - w0) with copy_span16.  The clip is what bounds the
//                        stores; a record may be cut at either end or at both.  Runs once per (batch, window) and reads nothing that
//                        depends on how many windows there are.  Every wave adds the bytes it wrote to a 64-bit counter with one
//                        atomic: the host refuses the window unless the counter shows the window's record bytes.
//
// The bin patch (fixbins): the copy SKIPS bytes 14 and 15 of a patched record -- the record is copied as [0, 14) and [16, len), two
// disjoint stretches clipped each on its own -- and lane 0 of the record's sixteen writes the two bytes, each only if it lies in
// [w0, w1).  So no byte of the window has two writers and the patch cannot race the copy, without the copy loop having to compare
// addresses per byte; the price is a second, 14-byte call of copy_span16 for the records that change, and none for those that do not
// (their bin is streamc::kNoPatch: one stretch).  PackArgs::patch_off moves the patched pair: 14 for the bin, 18 for the flag
// (subsample marks a dropped record there); the two stretches are then [0, patch_off) and [patch_off + 2, len).
//
// Bytes moved (a batch of n records, s of them selected, b selected bytes, written through k windows): K21a reads 32 n (descriptor)
// + 4 n (verdict) + 4 s scattered words of U and writes 4 n + 8 n / 256; K21b reads 4 n and writes 8 n; K21c reads, per window the
// batch meets, 12 n (dest, len) + 32 per record that has bytes in it (+ 4 with a patch), and over all its windows reads b and
// writes b.  No LDS atomics; LDS holds four words per workgroup in K21a and nothing in K21c.
#include "common.hpp"
#include "scan.hpp"
#include "stream.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

__global__ __launch_bounds__(kPackThreads) void k_pack_lengths(PackArgs a) {
    __shared__ unsigned long long w_sum[kPackThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kPackThreads + threadIdx.x;
    unsigned long long len = 0;
    if (i < a.n) {
        if (!a.count || a.count[i]) {
            const uint64_t rec_off = a.desc[i].rec_off;
            if (rec_off + 4 <= a.u_end) {
                const uint32_t bs = ld32(a.U + rec_off);
                if (record_len_ok(bs, rec_off, a.u_end)) len = bs + 4ull;
            }
        }
        a.len[i] = (uint32_t)len;
    }
    const unsigned long long all = block_sum<unsigned long long>(len, w_sum);
    if (threadIdx.x == 0) a.group_sum[blockIdx.x] = all;
}

static_assert(kPackThreads == kGroupThreads, "K21a sums the groups launch_group_offsets reads");

constexpr uint32_t kPackRecs = kPackThreads / kCopyGroup;

__global__ __launch_bounds__(kPackThreads) void k_pack_records(PackArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kPackRecs + threadIdx.x / kCopyGroup;
    const uint32_t l = threadIdx.x % kCopyGroup;
    unsigned long long wrote = 0;
    if (i < a.n) {
        const uint64_t len = a.len[i];
        const uint64_t d = a.dest[i];
        if (len && d < a.w1 && d + len > a.w0) {
            const uint8_t* rec = a.U + a.desc[i].rec_off;       // (K21a: the whole frame lies inside the batch)
            streamc::PackPlan p;
            streamc::plan_record(d, len, a.w0, a.w1, a.bin ? a.bin[i] : streamc::kNoPatch, &p, a.patch_off);
            for (uint32_t k = 0; k < p.n_spans; ++k) copy_span16(a.window + p.span[k].dst, rec + p.span[k].src, p.span[k].len, l);
            if (l == 0) {
                for (uint32_t k = 0; k < p.n_bytes; ++k) a.window[p.byte_dst[k]] = p.byte_val[k];
                wrote = p.wrote();
            }
        }
    }
    wrote = wave_sum(wrote);
    if ((threadIdx.x & 63u) == 0 && wrote) atomicAdd(a.acc, wrote);
}

}  // namespace

void launch_pack_offsets(const PackArgs& a, hipStream_t stream) {
    const uint32_t groups = pack_groups(a.n);
    if (a.n) {
        hipLaunchKernelGGL(k_pack_lengths, dim3(groups), dim3(kPackThreads), 0, stream, a);
        SBX_HIP(hipGetLastError());
    }
    launch_scan64(a.group_sum, groups, 0, stream);
    if (a.n) launch_group_offsets(a.len, a.group_sum, a.n, a.stream_base, a.dest, stream);
}

void launch_pack_records(const PackArgs& a, hipStream_t stream) {
    if (!a.n || a.w1 <= a.w0) return;
    const uint64_t groups = (a.n + kPackRecs - 1) / kPackRecs;
    hipLaunchKernelGGL(k_pack_records, dim3((uint32_t)groups), dim3(kPackThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
