// engine_windows.hpp -- what the windowed sort (engine_sort.cpp) and the streamed markdup (engine_markdup.cpp) share: a file larger
// than device memory, no record store.  The command's key pass saves its batches (for_each_record_batch with `saved`) and ends with
// one destination in the output stream per record.  From there on: the budget of device memory (WindowBudget), the stretch of the
// stream every saved batch goes to (BatchSpans), and write_windows -- the window chosen from what is free, then per window the saved
// batches that meet it once more through K1 + K2, the command's scatter kernel (K9d-3 / K10f: a callback), the two checks and the
// encoder of engine_stream.hpp into the file.  The words of the refusals are the command's (sortc::WindowWords).
#pragma once
#include "engine_store.hpp"

namespace sbx {

// ---- device memory: no store; the command's per-record arrays, one read batch, the encoder, one window ----
struct WindowBudget {
    const sortc::WindowWords* words;
    uint64_t hook;                      // the command's SBX_*_WINDOW_BYTES: windows of this many bytes (0: as large as fits)
    uint64_t u_total, u_first;          // inflated bytes of the file, offset of its first record
    uint64_t piece_blocks, piece_bytes; // (bgzf_piece_blocks(), read once for the call)
    uint64_t cap_bytes, out_reserve;    // the encoder's buffers, as plan_store_bytes reserves them
    uint64_t est_records;               // (as K2 sizes its descriptors)
    uint64_t batch_u = 0;               // inflated bytes per batch of the key pass: fit() sets it
    static constexpr uint64_t kMinBatch = 5ull * (64ull << 20);

    WindowBudget(sbx_ctx* c, uint64_t hlen, const sortc::WindowWords& w, uint64_t hook_) : words(&w), hook(hook_) {
        u_total = c->blocks.out_off.back();
        u_first = std::min<uint64_t>(c->hdr.first_record_off, u_total);
        piece_blocks = bgzf_piece_blocks();
        piece_bytes = piece_blocks * (uint64_t)kBgzfPayload;
        // the smallest window: one piece, or the whole stream when it is shorter
        cap_bytes = std::min<uint64_t>(piece_bytes, u_total - u_first + hlen + kBgzfPayload);
        out_reserve = cap_bytes * 3 + (8ull << 20);
        est_records = (u_total - u_first) / 160 + 4096;
    }
    // The first check, before the key pass: `kept` bytes of the command's own (its arrays at their peak), one batch of the smallest
    // size, the encoder and a window of one piece.  SBX_ENOMEM with `parts` between the brackets; otherwise the batch size follows.
    void fit(uint64_t kept, const std::string& parts) {
        size_t free_b = 0, total_b = 0;
        SBX_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t need = kept + kMinBatch + out_reserve + cap_bytes;
        if (need > free_b) throw Error(SBX_ENOMEM, sortc::windows_do_not_fit(*words, need, free_b, parts));
        batch_u = std::min<uint64_t>(index_batch_bytes(kept + out_reserve + cap_bytes), kWindowedBatchBytes);
    }
};

// ---- K9d-2: the stretch [lo, hi) of the stream every saved batch goes to; upload() in front of the caller's timer, launch() inside, read_back() behind ----
struct BatchSpans {
    const std::vector<SavedBatch>* saved = nullptr;
    std::vector<uint64_t> first, lo, hi;
    DevBuf<uint64_t> d_first, d_lo, d_hi;
    // n: records that take part; batch b holds [saved[b].first_kept, saved[b + 1].first_kept) of them
    void upload(const std::vector<SavedBatch>& batches, uint64_t n, hipStream_t s) {
        saved = &batches;
        first.assign(batches.size() + 1, n);
        for (size_t b = 0; b < batches.size(); ++b) first[b] = batches[b].first_kept;
        lo.assign(batches.size(), ~0ull);
        hi.assign(batches.size(), 0);
        d_first.alloc(first.size()); d_lo.alloc(batches.size() + 1); d_hi.alloc(batches.size() + 1);
        SBX_HIP(hipMemcpyAsync(d_first.p, first.data(), first.size() * 8, hipMemcpyHostToDevice, s));
    }
    // d_len: the length every record has in the output
    void launch(const uint64_t* d_dest, const uint32_t* d_len, hipStream_t s) {
        launch_batch_spans(d_dest, d_len, d_first.p, (uint32_t)saved->size(), d_lo.p, d_hi.p, s);
    }
    // lo / hi to the host; waits for the stream and frees the tables (the window is sized by what is free)
    void read_back(hipStream_t s) {
        if (!saved->empty()) {
            SBX_HIP(hipMemcpyAsync(lo.data(), d_lo.p, lo.size() * 8, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipMemcpyAsync(hi.data(), d_hi.p, hi.size() * 8, hipMemcpyDeviceToHost, s));
        }
        SBX_HIP(hipStreamSynchronize(s));
        d_first.release(); d_lo.release(); d_hi.release();
    }
};

// ---- the writer ----
struct WindowedOutput {
    uint32_t n_windows = 0, n_pieces = 0;
    uint64_t span = 0;                  // bytes per window (the last one may be shorter)
    uint64_t n_batch_runs = 0, n_batches_skipped = 0;
    double ms_scatter = 0, ms_inflate_replay = 0, ms_index_replay = 0;
    uint64_t compressed_bytes = 0;      // the file, EOF block included
    double ms_deflate = 0;              // deflate + packing of the blocks
    double w_planned = 0, w_written = 0;        // wall_now() in front of the first window; when the file is closed (the buffers still to free)
};
// The stream of `total` bytes -- `header`, then the records at their destinations -- into the file of `out`, window by window.  The
// window is what is free next to the batch buffers (they stay) less the encoder's, in whole pieces, or b.hook: the command releases
// what the windows do not need before the call.  scatter(saved batch, its records as they came this time, w, window, acc, stream)
// launches the command's kernel and nothing else: it puts bytes [w.w0, w.w1) of the stream at window[0, w.w1 - w.w0) and counts in
// acc[kWindowAccWords].  `out` is armed as soon as the file exists and stays armed.
template <class Scatter>
WindowedOutput write_windows(sbx_ctx* c, OutputGuard& out, const std::vector<uint8_t>& header, uint64_t total, const WindowBudget& b,
                             const BatchSpans& spans, int level, Scatter&& scatter) {
    const uint64_t hlen = header.size();
    hipStream_t s = c->stream.get();
    WindowedOutput r;
    const uint32_t cap_blocks = (uint32_t)std::min<uint64_t>(b.piece_blocks, std::max<uint64_t>(1, (total + kBgzfPayload - 1) / kBgzfPayload));
    uint64_t window_bytes = b.hook;
    if (!window_bytes) {
        size_t free_b = 0, total_b = 0;
        SBX_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t reserve = b.out_reserve + (64ull << 20);
        const uint64_t avail = free_b > reserve ? free_b - reserve : 0;
        const uint64_t smallest = std::min<uint64_t>(b.piece_bytes, total);
        if (avail < smallest) throw Error(SBX_ENOMEM, sortc::windows_do_not_fit(*b.words, smallest + reserve, free_b, b.words->window_needs));
        window_bytes = std::max<uint64_t>(avail / b.piece_bytes, 1) * b.piece_bytes;
    }
    const std::vector<sortc::Window> windows = sortc::plan_windows(total, b.piece_bytes, window_bytes);
    r.n_windows = (uint32_t)windows.size();
    r.span = sortc::window_span(b.piece_bytes, window_bytes);
    DevBuf<uint8_t> d_win((size_t)std::min<uint64_t>(r.span, total) + 64);
    DevBuf<unsigned long long> d_wacc(kWindowAccWords);
    BgzfPieceCompressor comp(cap_blocks, level, true);
    BgzfPieceTimes bt_times;
    r.w_planned = wall_now();

    OutputFile f(out);
    EventTimer t_s;
    for (const sortc::Window& w : windows) {
        SBX_HIP(hipMemsetAsync(d_wacc.p, 0, kWindowAccWords * sizeof(unsigned long long), s));
        if (w.w0 < hlen) SBX_HIP(hipMemcpyAsync(d_win.p, header.data() + w.w0, std::min<uint64_t>(hlen, w.w1) - w.w0, hipMemcpyHostToDevice, s));
        for (size_t k = 0; k < spans.saved->size(); ++k) {
            const SavedBatch& sb = (*spans.saved)[k];
            if (!sortc::span_meets_window(spans.lo[k], spans.hi[k], w.w0, w.w1)) { ++r.n_batches_skipped; continue; }
            ++r.n_batch_runs;
            run_record_batch(c, sb, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
                if (nrec != sb.nrec || base != sb.base || next != sb.next) throw Error(SBX_EIO, sortc::batch_refusal(*b.words));
                t_s.start(s);
                scatter(sb, RecordBatch{nrec, base, next}, w, d_win.p, d_wacc.p, s);
                t_s.stop(s);
                // (the next batch's K1 / K2 overwrite U and the descriptors: the scatter ends first)
                SBX_HIP(hipStreamSynchronize(s));
                r.ms_scatter += t_s.ms();
                r.ms_inflate_replay += c->stats.ms_inflate;
                r.ms_index_replay += c->stats.ms_index;
                return true;
            });
        }
        unsigned long long wacc[kWindowAccWords] = {0, 0};
        SBX_HIP(hipMemcpyAsync(wacc, d_wacc.p, sizeof wacc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        const std::string why = sortc::window_refusal(w.w0, w.w1, hlen, wacc[kWindowAccBytes], wacc[kWindowAccMismatch], *b.words);
        if (!why.empty()) throw Error(SBX_EIO, why);
        comp.run((size_t)(w.w1 - w.w0), false, &bt_times,
                 [&](uint8_t* d_in, size_t done, size_t bytes, hipStream_t ps) {
                     SBX_HIP(hipMemcpyAsync(d_in, d_win.p + done, bytes, hipMemcpyDeviceToDevice, ps));
                 },
                 [&](const uint8_t* p, size_t k) { f.write(p, k); });
    }
    f.finish(true);
    r.w_written = wall_now();
    r.n_pieces = bt_times.n_pieces;
    r.compressed_bytes = bt_times.out_bytes + sizeof kEofBlock;
    r.ms_deflate = bt_times.ms_deflate + bt_times.ms_pack;
    if (getenv("SBX_TIMING"))
        fprintf(stderr, "[sbx] output: stream_bytes=%llu compressed_bytes=%llu n_pieces=%u piece_blocks=%llu\n", (unsigned long long)total,
                (unsigned long long)r.compressed_bytes, r.n_pieces, (unsigned long long)b.piece_blocks);
    return r;
}

}  // namespace sbx
