// engine_stream.hpp -- the two streaming loops engine_writer.cpp and engine_sort.cpp share: BGZF compression of a byte stream piece by
// piece on the device (bgzf_compress_pieces: the source of a piece is a callback -- a copy from host memory for sbx_bgzf_compress /
// sbx_write_bam, a gather on the device for sbx_sort_bam) and the index-mode pass over the records of a file in batches
// (for_each_record_batch: sbx_build_index, sbx_flagstat, sbx_sort_bam; run_record_batch: one saved batch of such a pass once more,
// for the windowed sort).
#pragma once
#include <algorithm>
#include <cstdlib>

#include "deflate_core.hpp"
#include "engine_ctx.hpp"

namespace sbx {

constexpr size_t kBgzfPieceBlocks = 32768;      // BGZF blocks compressed per launch: a piece of the stream is at most this many payloads

// BGZF blocks per piece for one call: kBgzfPieceBlocks, or SBX_BGZF_PIECE_BLOCKS (tests: a decimal number, brought into
// [1, kBgzfPieceBlocks]; anything else counts as unset).  Blocks are cut every kBgzfPayload bytes whatever the piece, so the value
// does not change a byte of the output.  Read once per call: the caller hands the value to everything that depends on it.
inline size_t bgzf_piece_blocks() {
    return (size_t)std::min<uint64_t>(std::max<uint64_t>(env_u64("SBX_BGZF_PIECE_BLOCKS").value_or(kBgzfPieceBlocks), 1), kBgzfPieceBlocks);
}

struct BgzfPieceTimes { double ms_fill = 0, ms_deflate = 0, ms_pack = 0, ms_d2h = 0; uint64_t out_bytes = 0; uint32_t n_pieces = 0; };

// Compresses a stream of n bytes piece by piece on the device: pieces of piece_blocks (bgzf_piece_blocks()) payloads, the last one
// shorter.  fill(d_in, done, bytes, s) puts bytes [done, done + bytes) of the stream at d_in, in order on stream s; sink(data, len)
// receives consecutive pieces of the BGZF stream.  Blocks are cut every kBgzfPayload bytes.  pinned: the compressed piece travels
// through pinned host memory.  times (may be null) accumulates; the wall-clock figures (fill, device -> host) are taken only when
// `timing`, which synchronises after the fill.
// The buffers of one such stream; run() may be called again for further streams of at most cap_blocks payloads per piece (sbx_slice_bam
// compresses one short stream between every two stretches it copies from the file).
class BgzfPieceCompressor {
    Stream stream_;
    uint32_t cap_blocks_;
    int level_;
    bool pinned_;
    DevBuf<uint8_t> d_in_, d_slots_, d_out_;
    DevBuf<uint16_t> d_tab_;
    DevBuf<uint8_t> d_work_;
    DevBuf<uint32_t> d_len_;
    DevBuf<uint64_t> d_off_;
    std::vector<uint8_t> host_;
    PinnedBuf<uint8_t> host_pinned_;
    EventTimer t_def_, t_pack_;

public:
    BgzfPieceCompressor(uint32_t cap_blocks, int level, bool pinned)
        : cap_blocks_(cap_blocks), level_(level), pinned_(pinned), d_in_((size_t)cap_blocks * kBgzfPayload + 64),
          d_slots_((size_t)cap_blocks * kBgzfSlot), d_out_((size_t)cap_blocks * kBgzfSlot), d_tab_(deflate_table_entries(cap_blocks)),
          d_work_(deflate_work_bytes(cap_blocks)), d_len_(cap_blocks + 1), d_off_((size_t)cap_blocks + 2) {
        stream_.create();
    }
    template <class Fill, class Sink>
    void run(size_t n, bool timing, BgzfPieceTimes* times, Fill&& fill, Sink&& sink) {
        hipStream_t s = stream_.get();
        for (size_t done = 0; done < n;) {
            const size_t bytes = std::min<size_t>(n - done, (size_t)cap_blocks_ * kBgzfPayload);
            const uint32_t nb = (uint32_t)((bytes + kBgzfPayload - 1) / kBgzfPayload);
            const double w0 = wall_now();
            fill(d_in_.p, done, bytes, s);
            if (timing) SBX_HIP(hipStreamSynchronize(s));
            const double w1 = wall_now();
            t_def_.start(s);
            launch_bgzf_deflate(d_in_.p, bytes, nb, level_, d_slots_.p, d_tab_.p, d_work_.p, d_len_.p, s);
            t_def_.stop(s);
            t_pack_.start(s);
            launch_count_scan(d_len_.p, nb, d_off_.p, s);
            launch_pack_blocks(d_slots_.p, d_len_.p, d_off_.p, nb, d_out_.p, s);
            t_pack_.stop(s);
            uint64_t total = 0;
            SBX_HIP(hipMemcpyAsync(&total, d_off_.p + nb, 8, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            const double w2 = wall_now();
            uint8_t* h;
            if (pinned_) { host_pinned_.ensure((size_t)total + 1); h = host_pinned_.p; }
            else { host_.resize((size_t)total); h = host_.data(); }
            SBX_HIP(hipMemcpy(h, d_out_.p, (size_t)total, hipMemcpyDeviceToHost));
            if (times) {
                times->ms_deflate += t_def_.ms(); times->ms_pack += t_pack_.ms(); times->out_bytes += total; ++times->n_pieces;
                if (timing) { times->ms_fill += (w1 - w0) * 1e3; times->ms_d2h += (wall_now() - w2) * 1e3; }
            }
            sink(h, (size_t)total);
            done += bytes;
        }
    }
};

template <class Fill, class Sink>
void bgzf_compress_pieces(size_t n, size_t piece_blocks, int level, bool pinned, bool timing, BgzfPieceTimes* times, Fill&& fill, Sink&& sink) {
    const size_t n_blocks_total = (n + kBgzfPayload - 1) / kBgzfPayload;
    const uint32_t cap_blocks = (uint32_t)std::min<size_t>(piece_blocks, std::max<size_t>(1, n_blocks_total));
    BgzfPieceCompressor comp(cap_blocks, level, pinned);
    comp.run(n, timing, times, fill, sink);
}

// compresses in[0, n) (host memory) piece by piece on the device; sink(data, len) receives consecutive pieces of the BGZF stream
template <class Sink>
void bgzf_compress_stream(const uint8_t* in, size_t n, int level, Sink&& sink) {
    const bool timing = getenv("SBX_TIMING") != nullptr;
    BgzfPieceTimes t;
    bgzf_compress_pieces(n, bgzf_piece_blocks(), level, false, timing, &t,
                         [&](uint8_t* d_in, size_t done, size_t bytes, hipStream_t s) {
                             SBX_HIP(hipMemcpyAsync(d_in, in + done, bytes, hipMemcpyHostToDevice, s));
                         },
                         sink);
    if (timing)
        fprintf(stderr, "[sbx] bgzf_compress: %zu bytes -> %llu in %zu blocks, %u pieces: host -> device %.1f ms (pageable), deflate kernel %.1f ms (%.1f GB/s of input), "
                        "scan + pack %.1f ms, device -> host %.1f ms\n", n, (unsigned long long)t.out_bytes, (n + kBgzfPayload - 1) / kBgzfPayload, t.n_pieces,
                t.ms_fill, t.ms_deflate, t.ms_deflate > 0 ? (double)n / t.ms_deflate / 1e6 : 0.0, t.ms_pack, t.ms_d2h);
}

// ---- index-mode passes: the record stream of one file in batches (sbx_build_index, sbx_flagstat, sbx_sort_bam) ------------------------
// Inflated bytes per batch: a batch holds its compressed bytes, its inflated bytes, the token streams and the descriptors -- about
// five times its inflated size --, so the size follows the free device memory less `reserved` bytes the caller keeps for itself;
// SBX_INDEX_BATCH_BYTES overrides it (tests).
inline uint64_t index_batch_bytes(uint64_t reserved = 0) {
    uint64_t batch_u = 0;
    if (const char* e = getenv("SBX_INDEX_BATCH_BYTES")) batch_u = strtoull(e, nullptr, 10);
    if (!batch_u) {
        size_t free_b = 0, total_b = 0;
        SBX_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t avail = free_b > reserved ? free_b - reserved : 0;
        batch_u = std::max<uint64_t>(64ull << 20, (uint64_t)((double)avail * 0.7 / 5.0));
    }
    return batch_u;
}

// The file of an index-mode context goes through the device in batches of whole BGZF blocks -- inflate, record chain, descriptors.
// A batch ends in front of the record that straddles its last block boundary (ChainRun::open_end: the chain stops there and that
// record is not described) and the next batch starts with that record, so every record of the file is described in exactly one
// batch.  consume(nrec, base, next) is called once per batch: records [0, nrec) of c->d_desc / c->d_rec_ref are the batch's, their
// rec_off count from U[0] = inflated offset `base` of the file, and `next` is the inflated offset behind the batch's last record.
// It returns false to stop the pass (then so does this function); *n_batches receives the number of batches handed over.
//
// A batch is decided by (cur, bu) alone, so a pass can be repeated batch by batch: with `saved`, every batch handed over is also
// appended to it -- its run, what consume() received, and (cur, bu) -- and run_record_batch() below runs exactly that batch again.
// first_kept / n_kept are the caller's: the ordinal of the batch's first record that takes part and the number of those records.
struct SavedBatch {
    FileRun run;
    uint64_t cur, bu;               // the batch started at inflated offset cur with a batch size of bu bytes
    uint64_t nrec, base, next;      // what consume() received
    uint64_t first_kept = 0, n_kept = 0;
};
struct RecordBatch { uint64_t nrec, base, next; };
// K1 + K2 over one run of an index-mode context: the shared body of the pass and of its replay
inline RecordBatch describe_record_run(sbx_ctx* c, const FileRun& run) {
    const std::vector<FileRun> runs{run};
    run_impl(c, {}, false, &runs);
    RecordBatch b;
    b.nrec = c->primary_records;
    b.base = c->blocks.out_off[run.blk0];                // work-list offsets count from the batch's first block
    // an open-ended run stops in front of the record that straddles its last block boundary
    b.next = run.open_end && c->index_straddler != kOffUnknown ? b.base + c->index_straddler : run.ue;
    return b;
}
template <class Consume>
bool for_each_record_batch(sbx_ctx* c, uint64_t batch_u, uint32_t* n_batches, Consume&& consume, std::vector<SavedBatch>* saved = nullptr) {
    const BlockTable& bt = c->blocks;
    const size_t nbk = bt.size();
    const uint64_t total = bt.out_off.back(), first = c->hdr.first_record_off;
    uint64_t bu = batch_u;
    *n_batches = 0;
    for (uint64_t cur = first; cur < total;) {
        const uint32_t b0 = (uint32_t)(std::upper_bound(bt.out_off.begin(), bt.out_off.end(), cur) - bt.out_off.begin()) - 1;
        uint32_t b1 = (uint32_t)(std::lower_bound(bt.out_off.begin() + b0, bt.out_off.end(), bt.out_off[b0] + bu) - bt.out_off.begin());
        b1 = std::min<uint32_t>(std::max(b1, b0 + 1), (uint32_t)nbk);
        if (bt.out_off[b1] >= total) b1 = (uint32_t)nbk;          // (whatever follows holds no bytes: EOF blocks)
        const bool last = b1 == nbk;
        const FileRun run{b0, b1, cur, last ? total : bt.out_off[b1], !last};
        const RecordBatch b = describe_record_run(c, run);
        if (!last && b.next == cur) {                    // not one whole record in the batch: a longer batch
            bu *= 2;
            continue;
        }
        ++*n_batches;
        if (saved) saved->push_back(SavedBatch{run, cur, bu, b.nrec, b.base, b.next});
        if (!consume(b.nrec, b.base, b.next)) return false;
        cur = b.next;
    }
    return true;
}
// One batch of an earlier pass over the same context once more: the same run, hence the same U and the same descriptors at the same
// places.  consume(nrec, base, next) as above; what it returns is returned.  Whether the batch came out as it did the first time
// (b.nrec, b.base, b.next against the saved ones) is the consumer's to judge.
template <class Consume>
bool run_record_batch(sbx_ctx* c, const SavedBatch& saved, Consume&& consume) {
    const RecordBatch b = describe_record_run(c, saved.run);
    return consume(b.nrec, b.base, b.next);
}

}  // namespace sbx
