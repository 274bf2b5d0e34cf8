// engine_store.hpp -- what sbx_sort_bam, sbx_markdup, sbx_fixbins, sbx_merge_bam and sbx_view_bam share around their kernels.  Each of
// them reads as: checks, open (run_entry / open_record_pass / OutputGuard, engine_ctx.hpp), header, the decision between the resident
// record store and the path that keeps none, ONE batch step with the command's kernel that both paths call, order, output tail,
// stats line.  Here: the plan of the resident record store (1 x the inflated records of the file next to one batch of the read pass)
// and whether it fits (plan_if_fits / try_plan_record_store); PassBooks, the bookkeeping of a read pass (accumulators, the read-back
// that ends every batch step, the record count, the K1 / K2 times); the copy of a batch into the store; K9b over the keys of the
// resident records (sort and merge); and the output tail (write_store_output) that turns "header + records of the store in the order
// of a permutation" into a BGZF file piece by piece (offsets, piece bounds, K9c gather, deflate) and hands back the figures every
// stats struct takes.  The permutation is a list of record numbers: it may leave records out (a filter) or name one several times
// (sbx_view_bam with listed regions).  The stream written never exists as a whole.  What the kernels share is wave_prims.hpp.  A file
// that does not fit the store goes, for sort, markdup and merge, through engine_windows.hpp instead (the same reading order, a key pass for
// the plan, the windowed writer for the tail), for fixbins and view in file order through engine_streamout.hpp.
#pragma once
#include "engine_ctx.hpp"
#include "engine_stream.hpp"
#include "sort.hpp"
#include "sort_core.hpp"
#include <optional>

namespace sbx {

// "BAM\1", l_text, text, the binary reference list
inline std::vector<uint8_t> bam_header_bytes(const std::string& text, const std::vector<RefSeq>& refs) {
    std::vector<uint8_t> h;
    auto put32 = [&](uint32_t v) { for (int k = 0; k < 4; ++k) h.push_back((uint8_t)(v >> (8 * k))); };
    h.insert(h.end(), {'B', 'A', 'M', 1});
    put32((uint32_t)text.size());
    h.insert(h.end(), text.begin(), text.end());
    put32((uint32_t)refs.size());
    for (const RefSeq& r : refs) {
        put32((uint32_t)r.name.size() + 1);
        h.insert(h.end(), r.name.begin(), r.name.end());
        h.push_back(0);
        put32((uint32_t)r.length);
    }
    return h;
}

// a device array of the kept records that grows while the batches arrive (the number of records is not known in advance)
template <class T>
void grow_keeping(DevBuf<T>& b, size_t used, size_t want, hipStream_t s) {
    if (want <= b.n) return;
    DevBuf<T> nb(want + want / 2 + 1024);
    if (used) SBX_HIP(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
    SBX_HIP(hipStreamSynchronize(s));
    b = std::move(nb);
}

// ---- device memory: the record store, the per-record arrays, one read batch, one output piece ----
struct StorePlan {
    uint64_t u_total, u_first;      // inflated bytes of the file, offset of its first record
    uint64_t store_bytes;           // the records
    uint64_t est_records;           // (as K2 sizes its descriptors; the arrays grow when it is more)
    uint64_t fixed_need;            // store + per-record arrays
    uint64_t batch_u;               // inflated bytes per batch of the read pass
};
// store_bytes: the records that stay resident (for several inputs: their sum, plus what rewriting may add); hlen: bytes of the output
// header; per_record: bytes of per-record arrays the command keeps; doing: "sorting" (for the refusal); what: "the file does" / "the files do".
// SBX_ENOMEM when they do not fit the device.
inline StorePlan plan_store_bytes(uint64_t store_bytes, uint64_t hlen, uint64_t per_record, const char* doing, const char* what) {
    StorePlan p{};
    p.store_bytes = store_bytes;
    p.est_records = p.store_bytes / 160 + 4096;
    const uint64_t piece_bytes = std::min<uint64_t>(kBgzfPieceBlocks * (uint64_t)kBgzfPayload, p.store_bytes + hlen + kBgzfPayload);
    const uint64_t out_reserve = piece_bytes * 3 + (8ull << 20);    // piece, slots, packed blocks (kBgzfSlot ~ kBgzfPayload)
    p.fixed_need = p.store_bytes + p.est_records * per_record;
    size_t free_b = 0, total_b = 0;
    SBX_HIP(hipMemGetInfo(&free_b, &total_b));
    const uint64_t min_batch = 5ull * (64ull << 20);
    if (p.fixed_need + std::max(out_reserve, min_batch) > free_b)
        throw Error(SBX_ENOMEM, std::string(what) + " not fit the device: " + doing + " it needs " +
                                    std::to_string(p.fixed_need + std::max(out_reserve, min_batch)) + " bytes of device memory (" +
                                    std::to_string(p.store_bytes) + " of inflated records resident), " + std::to_string(free_b) +
                                    " are free; an out-of-core merge is not implemented");
    p.batch_u = index_batch_bytes(p.fixed_need);
    return p;
}
// one input: the store holds its inflated records
inline StorePlan plan_record_store(sbx_ctx* c, uint64_t hlen, uint64_t per_record, const char* doing) {
    const uint64_t u_total = c->blocks.out_off.back(), u_first = std::min<uint64_t>(c->hdr.first_record_off, u_total);
    StorePlan p = plan_store_bytes(u_total - u_first, hlen, per_record, doing, "the file does");
    p.u_total = u_total;
    p.u_first = u_first;
    return p;
}

// The resident-or-not decision: the plan, or nothing when the store does not fit the device.  Only SBX_ENOMEM means that; every
// other error passes through.  A command that has no other path (sort -n / -N / -M) calls plan_* itself and keeps the refusal.
template <class Plan>
std::optional<StorePlan> plan_if_fits(Plan&& plan) {
    try {
        return plan();
    } catch (const Error& e) {
        if (e.code != SBX_ENOMEM) throw;
        return std::nullopt;
    }
}
inline std::optional<StorePlan> try_plan_record_store(sbx_ctx* c, uint64_t hlen, uint64_t per_record, const char* doing) {
    return plan_if_fits([&] { return plan_record_store(c, hlen, per_record, doing); });
}

// ---- what every read pass keeps next to its kernel ----
// The N accumulator words of the command's kernel on the device and their host mirror, the records of the batches so far with the
// refusal of more than 0xFFFFFFF0 of them, and the K1 / K2 times of the batches.  A batch step ends with read_back(): when it
// returns the stream is idle, so the next batch's K1 / K2 may overwrite U and the descriptors.
template <size_t N>
struct PassBooks {
    DevBuf<unsigned long long> d_acc{N};
    unsigned long long acc[N] = {0};
    uint64_t n = 0;                 // records of the batches that were read back
    bool too_many = false;
    double ms_inflate = 0, ms_index = 0;
    // acc[] -- all 0, or what the caller has put there (sort's are not all 0) -- goes to the device
    void init(hipStream_t s) {
        SBX_HIP(hipMemcpyAsync(d_acc.p, acc, sizeof acc, hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));
    }
    // in front of a batch of nrec records: false when the pass has to stop because there are too many (refuse_too_many() says so)
    bool admit(uint64_t nrec) {
        too_many = too_many || n + nrec > 0xFFFFFFF0ull;
        return !too_many;
    }
    // the end of a batch step: the accumulators as the kernels queued on s leave them, the batch's records and K1 / K2 times added
    void read_back(sbx_ctx* c, uint64_t nrec, hipStream_t s) {
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        ms_inflate += c->stats.ms_inflate;
        ms_index += c->stats.ms_index;
        n += nrec;
    }
    // kept: records that take part, for a command that counts those (sort)
    void refuse_too_many(uint64_t kept = 0) const {
        if (too_many || kept > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
    }
};

// the records of a batch (for_each_record_batch: inflated offsets [cur, next), U[0] = offset `base`) go behind those of the batches before
inline void copy_batch_to_store(sbx_ctx* c, uint8_t* d_store, uint64_t u_first, uint64_t cur, uint64_t base, uint64_t next, hipStream_t s) {
    if (next > cur) SBX_HIP(hipMemcpyAsync(d_store + (cur - u_first), c->U() + (cur - base), next - cur, hipMemcpyDeviceToDevice, s));
}

// Inflated bytes per batch of the paths that keep no record store (the windowed sort, the streamed markdup).  The batch buffers
// (~5 x this) stay allocated from the key pass to the last window and are taken from what the windows could have: a batch is kept
// small against a window, and a short batch has a narrow span of destinations, which is what lets a window skip it.  K1 + K2 run at
// ~300 GB/s of inflated bytes (README), so 2 GiB is ~7 ms of kernels per batch -- far above the cost of launching them.
constexpr uint64_t kWindowedBatchBytes = 2ull << 30;

// ---- K9b over the keys of the resident records ----
struct ResidentOrder {
    DevBuf<uint64_t> key2;          // the second key buffer; free for the output offsets once the sort is done
    DevBuf<uint32_t> val, val2;
    const uint32_t* perm = nullptr; // [n] record numbers in key order, equal keys in the order they had (one of val / val2)
    uint32_t key_bits = 0, n_passes = 0;
    double ms_sort = 0;
    DevBuf<uint32_t> hist;          // K9b's counters and their scan
    DevBuf<uint64_t> hist_base;
};
// The buffers of an order over n resident records
inline void alloc_resident_order(uint64_t n, ResidentOrder* o) {
    o->key2 = DevBuf<uint64_t>((size_t)n + 2);
    o->val = DevBuf<uint32_t>((size_t)n + 2);
    o->val2 = DevBuf<uint32_t>((size_t)n + 2);
    o->hist = DevBuf<uint32_t>(radix_hist_entries(n) + 4);
    o->hist_base = DevBuf<uint64_t>(radix_hist_entries(n) + 4);
}
// K9b from the permutation the order holds: d_key[i] (n + 2 words; overwritten) is the key of record o->perm[i].  The passes over the
// key bits that vary (`varying` = OR of the keys ^ AND of the keys) are queued on s; o->perm, key_bits and n_passes follow.
inline void queue_resident_passes(uint64_t* d_key, uint64_t n, uint64_t varying, hipStream_t s, ResidentOrder* o) {
    uint32_t shifts[8], bits = 0;
    const uint32_t n_passes = n ? sortc::plan_passes(varying, shifts, &bits) : 0;
    uint64_t* keys[2] = {d_key, o->key2.p};
    uint32_t* vals[2] = {o->val.p, o->val2.p};
    int at = 0, vat = o->perm == o->val2.p ? 1 : 0;
    for (uint32_t p = 0; p < n_passes; ++p, at ^= 1, vat ^= 1)
        launch_radix_pass(keys[at], vals[vat], keys[at ^ 1], vals[vat ^ 1], n, shifts[p], o->hist.p, o->hist_base.p, s);
    o->perm = vals[vat];
    o->key_bits += bits;
    o->n_passes += n_passes;
}
// Stable radix sort of d_key[0, n) (n + 2 words; overwritten), the key of record i at d_key[i], over the key bits that vary.
inline void sort_resident(uint64_t* d_key, uint64_t n, uint64_t varying, hipStream_t s, ResidentOrder* o) {
    alloc_resident_order(n, o);
    EventTimer t_sort;
    t_sort.start(s);
    launch_iota(o->val.p, n, s);
    o->perm = o->val.p;
    queue_resident_passes(d_key, n, varying, s, o);
    t_sort.stop(s);
    SBX_HIP(hipStreamSynchronize(s));
    o->hist.release();
    o->hist_base.release();
    o->ms_sort = t_sort.ms();
}
// The same sort for a key of several words, one call per word, the least significant first: begin_resident_order sets the identity,
// every continue_resident_order sorts by one more word (d_key[i]: that word of record o->perm[i]) and keeps the order records with
// equal words had.  key_bits, n_passes and ms_sort add up over the calls.
inline void begin_resident_order(uint64_t n, hipStream_t s, ResidentOrder* o) {
    alloc_resident_order(n, o);
    EventTimer t;
    t.start(s);
    launch_iota(o->val.p, n, s);
    t.stop(s);
    o->perm = o->val.p;
    o->ms_sort += t.ms();
}
inline void continue_resident_order(uint64_t* d_key, uint64_t n, uint64_t varying, hipStream_t s, ResidentOrder* o) {
    EventTimer t;
    t.start(s);
    queue_resident_passes(d_key, n, varying, s, o);
    t.stop(s);
    o->ms_sort += t.ms();
}

// ---- the reference names on the device (K13, K15): name r is bytes[off[r], off[r + 1]) ----
struct DeviceRefNames {             // (the host side stays alive with the copies queued from it)
    std::vector<uint32_t> h_off{0};
    std::string h_bytes;
    DevBuf<uint32_t> off;
    DevBuf<char> bytes;
    int32_t n() const { return (int32_t)h_off.size() - 1; }
};
inline void upload_ref_names(const std::vector<RefSeq>& refs, hipStream_t s, DeviceRefNames* d) {
    for (const RefSeq& q : refs) { d->h_bytes += q.name; d->h_off.push_back((uint32_t)d->h_bytes.size()); }
    d->off.alloc(d->h_off.size());
    d->bytes.alloc(d->h_bytes.size() + 1);
    SBX_HIP(hipMemcpyAsync(d->off.p, d->h_off.data(), d->h_off.size() * 4, hipMemcpyHostToDevice, s));
    if (!d->h_bytes.empty()) SBX_HIP(hipMemcpyAsync(d->bytes.p, d->h_bytes.data(), d->h_bytes.size(), hipMemcpyHostToDevice, s));
}

// ---- the writer ----
struct OutputPlan {
    uint64_t total = 0;             // bytes of the stream: header + records
    uint64_t piece_blocks = 0;      // BGZF payloads per piece (bgzf_piece_blocks(), read once for the call)
    std::vector<uint32_t> bounds;   // the first record that ends behind byte k * piece_bytes()
    uint64_t piece_bytes() const { return piece_blocks * (uint64_t)kBgzfPayload; }
};
// Offsets of the records d_perm[0, n) in the output stream (d_out_off[0, n], n + 2 words) and the records at the piece boundaries.
// *ms_gather += device time of the offsets.
inline OutputPlan plan_output(const uint32_t* d_len, const uint32_t* d_perm, uint64_t n, uint64_t hlen, uint64_t* d_out_off, hipStream_t s,
                              double* ms_gather) {
    OutputPlan p;
    p.total = hlen;
    p.piece_blocks = bgzf_piece_blocks();
    EventTimer t;
    DevBuf<uint64_t> d_tile_sum(len_tiles(n) + 2);
    t.start(s);
    launch_sorted_offsets(d_len, d_perm, n, hlen, d_tile_sum.p, d_out_off, s);
    t.stop(s);
    if (n) SBX_HIP(hipMemcpyAsync(&p.total, d_out_off + n, 8, hipMemcpyDeviceToHost, s));
    SBX_HIP(hipStreamSynchronize(s));
    if (n) *ms_gather += t.ms();                        // (the offsets are the gather's preparation)
    const uint64_t cap = p.piece_bytes();
    const uint32_t n_bounds = (uint32_t)((p.total + cap - 1) / cap) + 1;
    p.bounds.assign(n_bounds, (uint32_t)n);
    if (n) {
        DevBuf<uint32_t> d_bounds(n_bounds);
        launch_piece_bounds(d_out_off, n, cap, n_bounds, d_bounds.p, s);
        SBX_HIP(hipMemcpyAsync(p.bounds.data(), d_bounds.p, (size_t)n_bounds * 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
    }
    return p;
}

// K9c + deflate, piece by piece, into the file of `out` (+ the EOF block).  `out` is armed as soon as the file exists: it removes
// the file when the call, or the command after it, fails.
inline void write_permuted_bam(OutputGuard& out, const std::vector<uint8_t>& header, const OutputPlan& plan, const uint8_t* d_store,
                               const uint64_t* d_off, const uint32_t* d_perm, const uint64_t* d_out_off, uint64_t n, int level,
                               double* ms_gather, BgzfPieceTimes* bt_times) {
    const uint64_t hlen = header.size();
    OutputFile f(out);
    EventTimer t_gather;
    bgzf_compress_pieces((size_t)plan.total, (size_t)plan.piece_blocks, level, true, false, bt_times,
                         [&](uint8_t* d_in, size_t done, size_t bytes, hipStream_t ps) {
                             const uint64_t p0 = done, p1 = done + bytes;
                             const size_t k = (size_t)(p0 / plan.piece_bytes());
                             t_gather.start(ps);
                             if (p0 < hlen) {
                                 const uint64_t he = std::min<uint64_t>(hlen, p1);
                                 SBX_HIP(hipMemcpyAsync(d_in, header.data() + p0, he - p0, hipMemcpyHostToDevice, ps));
                             }
                             uint64_t r0, r1;
                             sortc::piece_records(plan.bounds.data(), k, n, &r0, &r1);
                             launch_gather_records(d_store, d_off, d_perm, d_out_off, r0, r1, p0, p1, d_in, ps);
                             t_gather.stop(ps);
                             *ms_gather += t_gather.ms();
                         },
                         [&](const uint8_t* p, size_t k) { f.write(p, k); });
    f.finish(true);
}

// ---- the output tail of the four commands ----
struct WrittenBam {
    uint64_t stream_bytes = 0;      // header + records, inflated
    uint64_t compressed_bytes = 0;  // the file, EOF block included
    double ms_deflate = 0;          // deflate + packing of the blocks
    double w_planned = 0;           // wall_now() between the offsets and the first piece
};
// The records d_perm[0, n) of the store, behind `header`, into the file of `out`: offsets (plan_output, into d_out_off: n + 2 words
// the caller provides -- sort and merge hand in a key buffer they are done with), the check that they add up to *expect_bytes record
// bytes (null: no check; `records` words the refusal: "sorted records"), d_len released, K9c + deflate.  *ms_gather += device time
// of offsets and gather.  `out` stays armed: the caller disarms it when nothing can fail any more.
inline WrittenBam write_store_output(OutputGuard& out, const std::vector<uint8_t>& header, const uint8_t* d_store, const uint64_t* d_off,
                                     DevBuf<uint32_t>& d_len, const uint32_t* d_perm, uint64_t n, uint64_t* d_out_off, int level,
                                     const unsigned long long* expect_bytes, const char* records, hipStream_t s, double* ms_gather) {
    WrittenBam w;
    const OutputPlan plan = plan_output(d_len.p, d_perm, n, header.size(), d_out_off, s, ms_gather);
    if (expect_bytes && plan.total != header.size() + *expect_bytes)
        throw Error(SBX_EFORMAT, std::string("internal error: the offsets of the ") + records + " do not add up");
    d_len.release();
    w.w_planned = wall_now();
    BgzfPieceTimes bt_times;
    write_permuted_bam(out, header, plan, d_store, d_off, d_perm, d_out_off, n, level, ms_gather, &bt_times);
    w.stream_bytes = plan.total;
    w.compressed_bytes = bt_times.out_bytes + 28;
    w.ms_deflate = bt_times.ms_deflate + bt_times.ms_pack;
    if (getenv("SBX_TIMING"))
        fprintf(stderr, "[sbx] output: stream_bytes=%llu compressed_bytes=%llu n_pieces=%u piece_blocks=%llu\n", (unsigned long long)w.stream_bytes,
                (unsigned long long)w.compressed_bytes, bt_times.n_pieces, (unsigned long long)plan.piece_blocks);
    return w;
}

// the .bai next to a BAM just written: a pass of its own, not part of the command's figures; a failure leaves the BAM in place
inline int index_written_bam(const char* path, int with_index, int device, char* err, size_t errlen) {
    if (!with_index) return SBX_OK;
    return sbx_build_index(path, (std::string(path) + ".bai").c_str(), device, err, errlen);
}

}  // namespace sbx
