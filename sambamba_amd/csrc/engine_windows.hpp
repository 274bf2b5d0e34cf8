// engine_windows.hpp -- what the windowed sort (engine_sort.cpp), the streamed markdup (engine_markdup.cpp) and the windowed merge
// (engine_merge.cpp) share: input larger than device memory, no record store.  The command's key pass saves its batches
// (for_each_record_batch with `saved`) and ends with one destination in the output stream per record.  From there on: the budget of
// device memory (WindowBudget), the stretch of the stream every saved batch goes to (BatchSpans), and write_windows -- the window
// chosen from what is free, then per window the saved batches that meet it once more through K1 + K2, the command's scatter kernel
// (K9d-3 / K10f / K11c: a callback), the two checks and the encoder of engine_stream.hpp into the file.  The words of the refusals
// are the command's (sortc::WindowWords).
//
// The records come from a LIST OF SOURCES (WindowSource): one input file each, with a way to obtain its open record-pass context,
// the batches its key pass saved and its share of the ordinals.  Sort and markdup have one source whose context is open from the
// key pass on (one_open_source); merge has one per input, and at most one of them is open at a time.
#pragma once
#include <functional>

#include "engine_store.hpp"

namespace sbx {

// ---- one input of the windowed writer ----
struct WindowSource {
    std::function<sbx_ctx*()> open;     // the input's record-pass context, opened for the call when it is not open
    std::function<void()> close;        // the writer is done with the context for now (a source that stays open does nothing)
    const std::vector<SavedBatch>* saved = nullptr;     // the batches of its key pass; first_kept counts over ALL sources
    uint64_t first_ordinal = 0, n_ordinals = 0;         // its share of the ordinals: [first_ordinal, first_ordinal + n_ordinals)
};
// the one source of a command with one input whose context `c` stays open; n: records that take part
inline std::vector<WindowSource> one_open_source(sbx_ctx* c, const std::vector<SavedBatch>& saved, uint64_t n) {
    WindowSource src;
    src.open = [c] { return c; };
    src.close = [] {};
    src.saved = &saved;
    src.n_ordinals = n;
    return {src};
}

// A saved batch can be run again on `c` only while the block table of `c` still holds the run's blocks where the key pass found
// them: a source that is opened again for the windows (merge) may meet a file that was truncated or replaced meanwhile, and the
// work list indexes the table by the saved block numbers.  Host only; false is the batch_refusal of the command.
inline bool saved_run_fits(const sbx_ctx* c, const SavedBatch& sb) {
    const BlockTable& bt = c->blocks;
    const FileRun& r = sb.run;
    if (r.blk0 >= r.blk1 || r.blk1 > bt.size() || bt.out_off.size() != bt.size() + 1) return false;
    return bt.out_off[r.blk0] == sb.base && r.ub >= sb.base && r.ub <= r.ue && r.ue == (r.open_end ? bt.out_off[r.blk1] : bt.out_off.back());
}

// ---- device memory: no store; the command's per-record arrays, one read batch, the encoder, one window ----
struct WindowBudget {
    const sortc::WindowWords* words;
    uint64_t hook;                      // the command's SBX_*_WINDOW_BYTES: windows of this many bytes (0: as large as fits)
    uint64_t u_total, u_first;          // inflated bytes of the input (summed over the inputs), offset of the first record (one input)
    uint64_t piece_blocks, piece_bytes; // (bgzf_piece_blocks(), read once for the call)
    uint64_t cap_bytes, out_reserve;    // the encoder's buffers, as plan_store_bytes reserves them
    uint64_t est_records;               // (as K2 sizes its descriptors; summed over the inputs)
    uint64_t batch_u = 0;               // inflated bytes per batch of the key pass: fit() sets it
    uint64_t batch_reserve = 0;         // bytes the batch buffers will take when the windows come and no source is open (0: they are allocated)
    static constexpr uint64_t kMinBatch = 5ull * (64ull << 20);

    // record_bytes: inflated bytes of the records of all inputs
    WindowBudget(uint64_t u_total_, uint64_t u_first_, uint64_t record_bytes, uint64_t hlen, const sortc::WindowWords& w, uint64_t hook_)
        : words(&w), hook(hook_), u_total(u_total_), u_first(u_first_) {
        piece_blocks = bgzf_piece_blocks();
        piece_bytes = piece_blocks * (uint64_t)kBgzfPayload;
        // the smallest window: one piece, or the whole stream when it is shorter
        cap_bytes = std::min<uint64_t>(piece_bytes, record_bytes + hlen + kBgzfPayload);
        out_reserve = cap_bytes * 3 + (8ull << 20);
        est_records = record_bytes / 160 + 4096;
    }
    // one input
    WindowBudget(sbx_ctx* c, uint64_t hlen, const sortc::WindowWords& w, uint64_t hook_)
        : WindowBudget(c->blocks.out_off.back(), std::min<uint64_t>(c->hdr.first_record_off, c->blocks.out_off.back()),
                       c->blocks.out_off.back() - std::min<uint64_t>(c->hdr.first_record_off, c->blocks.out_off.back()), hlen, w, hook_) {}
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
// The batches of all sources are numbered source by source: batch j of source k is start[k] + j.
struct BatchSpans {
    std::vector<size_t> start;          // [sources + 1]
    std::vector<uint64_t> first, lo, hi;
    DevBuf<uint64_t> d_first, d_lo, d_hi;
    size_t n_batches() const { return lo.size(); }
    // n: records that take part; a batch holds the ordinals from its first_kept to the next batch's (of any source), the last one to n
    void upload(const std::vector<WindowSource>& sources, uint64_t n, hipStream_t s) {
        start.assign(1, 0);
        first.clear();
        for (const WindowSource& src : sources) {
            for (const SavedBatch& b : *src.saved) first.push_back(b.first_kept);
            start.push_back(first.size());
        }
        first.push_back(n);
        lo.assign(first.size() - 1, ~0ull);
        hi.assign(first.size() - 1, 0);
        d_first.alloc(first.size()); d_lo.alloc(lo.size() + 1); d_hi.alloc(hi.size() + 1);
        SBX_HIP(hipMemcpyAsync(d_first.p, first.data(), first.size() * 8, hipMemcpyHostToDevice, s));
    }
    // d_len: the length every record has in the output
    void launch(const uint64_t* d_dest, const uint32_t* d_len, hipStream_t s) {
        launch_batch_spans(d_dest, d_len, d_first.p, (uint32_t)n_batches(), d_lo.p, d_hi.p, s);
    }
    // lo / hi to the host; waits for the stream and frees the tables (the window is sized by what is free)
    void read_back(hipStream_t s) {
        if (n_batches()) {
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
    uint64_t n_input_opens = 0;         // times a source's context was asked for because another one (or none) was open
    double ms_scatter = 0, ms_inflate_replay = 0, ms_index_replay = 0;
    uint64_t compressed_bytes = 0;      // the file, EOF block included
    double ms_deflate = 0;              // deflate + packing of the blocks
    double w_planned = 0, w_written = 0;        // wall_now() in front of the first window; when the file is closed (the buffers still to free)
};
// The stream of `total` bytes -- `header`, the source-independent prefix, then the records at their destinations -- into the file of
// `out`, window by window.  The window is what is free next to the batch buffers (they stay, or b.batch_reserve stands for them)
// less the encoder's, in whole pieces, or b.hook: the command releases what the windows do not need before the call.  Per window
// the sources are visited in input order; a source none of whose batch spans meets the window is not opened for it, and a source
// is closed before another one is opened, so the batch buffers of two contexts are never on the device together.  s: the stream
// of the writer's own copies (for one open source: its context's).  scatter(index of the source, its context, saved batch, its
// records as they came this time, w, window, acc, the context's stream) launches the command's kernel and nothing else: it puts
// bytes [w.w0, w.w1) of the stream at window[0, w.w1 - w.w0) and counts in acc[kWindowAccWords].  `out` is armed as soon as the
// file exists and stays armed.
template <class Scatter>
WindowedOutput write_windows(const std::vector<WindowSource>& sources, hipStream_t s, OutputGuard& out, const std::vector<uint8_t>& header,
                             uint64_t total, const WindowBudget& b, const BatchSpans& spans, int level, Scatter&& scatter) {
    const uint64_t hlen = header.size();
    WindowedOutput r;
    const uint32_t cap_blocks = (uint32_t)std::min<uint64_t>(b.piece_blocks, std::max<uint64_t>(1, (total + kBgzfPayload - 1) / kBgzfPayload));
    uint64_t window_bytes = b.hook;
    if (!window_bytes) {
        size_t free_b = 0, total_b = 0;
        SBX_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t reserve = b.out_reserve + (64ull << 20) + b.batch_reserve;
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

    // the one source whose context is open; closed when another is needed, when the windows are done and when an error unwinds
    struct OpenSource {
        const std::vector<WindowSource>& sources;
        size_t at = ~(size_t)0;
        sbx_ctx* c = nullptr;
        void close() {
            if (c) sources[at].close();
            c = nullptr;
        }
        ~OpenSource() { close(); }
    } open{sources};

    OutputFile f(out);
    EventTimer t_s;
    for (const sortc::Window& w : windows) {
        SBX_HIP(hipMemsetAsync(d_wacc.p, 0, kWindowAccWords * sizeof(unsigned long long), s));
        if (w.w0 < hlen) SBX_HIP(hipMemcpyAsync(d_win.p, header.data() + w.w0, std::min<uint64_t>(hlen, w.w1) - w.w0, hipMemcpyHostToDevice, s));
        bool writer_idle = false;       // (a context with a stream of its own starts when the copies above have ended)
        for (size_t src = 0; src < sources.size(); ++src) {
            const std::vector<SavedBatch>& saved = *sources[src].saved;
            for (size_t j = 0; j < saved.size(); ++j) {
                const SavedBatch& sb = saved[j];
                const size_t k = spans.start[src] + j;
                if (!sortc::span_meets_window(spans.lo[k], spans.hi[k], w.w0, w.w1)) { ++r.n_batches_skipped; continue; }
                ++r.n_batch_runs;
                if (!open.c || open.at != src) {
                    open.close();
                    open.at = src;
                    open.c = sources[src].open();
                    ++r.n_input_opens;
                }
                sbx_ctx* c = open.c;
                if (!saved_run_fits(c, sb)) throw Error(SBX_EIO, sortc::batch_refusal(*b.words));
                hipStream_t cs = c->stream.get();
                if (cs != s && !writer_idle) {
                    SBX_HIP(hipStreamSynchronize(s));
                    writer_idle = true;
                }
                run_record_batch(c, sb, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
                    if (nrec != sb.nrec || base != sb.base || next != sb.next) throw Error(SBX_EIO, sortc::batch_refusal(*b.words));
                    t_s.start(cs);
                    scatter(src, c, sb, RecordBatch{nrec, base, next}, w, d_win.p, d_wacc.p, cs);
                    t_s.stop(cs);
                    // (the next batch's K1 / K2 overwrite U and the descriptors: the scatter ends first)
                    SBX_HIP(hipStreamSynchronize(cs));
                    r.ms_scatter += t_s.ms();
                    r.ms_inflate_replay += c->stats.ms_inflate;
                    r.ms_index_replay += c->stats.ms_index;
                    return true;
                });
            }
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
    open.close();
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
