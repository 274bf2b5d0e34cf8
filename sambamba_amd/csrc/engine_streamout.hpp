// engine_streamout.hpp -- StreamedOutput: the writer of the commands whose output order is the input order (view with the BAM sink,
// fixbins) for a file whose records do not fit the device.  No record store, no key pass, no replay: K1 + K2 run once, and while a
// batch is in U the consumer hands it over -- K21 (stream.hip) puts its selected records into ONE staging window of the output stream,
// a full window goes through the encoder of engine_stream.hpp into the file, the window moves on and K21 runs again on the same
// batch until the batch is consumed.  The window is a whole number of compression pieces and BGZF blocks are cut every kBgzfPayload
// bytes of the stream, so the file is the resident path's byte for byte.  The encoder runs between two launches of K21; overlapping
// them through a second window is a follow-up.  sbx_import_sam (engine_import.cpp) uses the same writer with
// fillers of its own and no known bound of the stream: take() with K15d (samparse.hip) for the records of a text chunk, take_device()
// for the records it had kept in a store before it found that they do not fit.
// The SAM sink of view streams too, but needs none of this: its text goes piece by piece through the buffers of the resident sink
// (engine_view.cpp, view_sam_streamed); of this file it uses StreamBudget's second form and the hook.
#pragma once
#include "engine_store.hpp"
#include "stream.hpp"

namespace sbx {

// SBX_STREAM_WINDOW_BYTES (tests, measurements): the streamed path is taken and its window is this many bytes, rounded up to whole
// pieces.  Anything that is not a positive decimal counts as unset (0).
inline uint64_t stream_window_hook() { return env_size("SBX_STREAM_WINDOW_BYTES", 0); }

// ---- device memory: one read batch, the per-batch arrays, the encoder, one window ----
struct StreamBudget {
    uint64_t piece_blocks, piece_bytes;     // (bgzf_piece_blocks(), read once for the call)
    uint64_t cap_bytes, out_reserve;        // the encoder's buffers, as plan_store_bytes reserves them
    uint64_t window_bytes = 0;              // whole pieces
    uint64_t batch_u = 0;                   // inflated bytes per batch of the read pass
    static constexpr uint64_t kMinBatch = 5ull * (64ull << 20);

    // stream_max: no more bytes than this are written (header + every record the pass reads); hook: stream_window_hook();
    // per_record: bytes of the arrays the command and K21 keep per record of a batch (`arrays` words them in the refusal);
    // doing: "selecting records of" / "fixing the bins of"; hint: a sentence behind the refusal, or "".
    // SBX_ENOMEM unless one batch of the smallest size with its arrays, the encoder and a window of one piece fit.
    StreamBudget(uint64_t stream_max, uint64_t hook, uint64_t per_record, const char* doing, const char* arrays, const char* hint) {
        init(stream_max, hook, per_record, true, 0, doing, arrays, hint);
    }
    // The same for a sink that has neither window nor encoder (the SAM text of view): `fixed` bytes of its own next to the batch.
    StreamBudget(uint64_t fixed, uint64_t per_record, const char* doing, const char* arrays, const char* hint) {
        init(0, 0, per_record, false, fixed, doing, arrays, hint);
    }

private:
    void init(uint64_t stream_max, uint64_t hook, uint64_t per_record, bool windowed, uint64_t fixed, const char* doing, const char* arrays,
              const char* hint) {
        piece_blocks = bgzf_piece_blocks();
        piece_bytes = piece_blocks * (uint64_t)kBgzfPayload;
        cap_bytes = windowed ? std::min<uint64_t>(piece_bytes, stream_max + kBgzfPayload) : 0;
        out_reserve = windowed ? cap_bytes * 3 + (8ull << 20) : fixed;
        size_t free_b = 0, total_b = 0;
        SBX_HIP(hipMemGetInfo(&free_b, &total_b));
        // (a minimal batch inflates to kMinBatch / 5 bytes; records as K2 estimates them)
        const uint64_t min_arrays = (kMinBatch / 5 / 160 + 4096) * per_record;
        const uint64_t need = kMinBatch + min_arrays + out_reserve + cap_bytes;
        if (need > free_b)
            throw Error(SBX_ENOMEM, std::string("the file does not fit the device: ") + doing + " it in a stream needs " + std::to_string(need) +
                                        " bytes of device memory (one read batch, " + arrays +
                                        (windowed ? ", the encoder and a window of one piece), " : "), ") +
                                        std::to_string(free_b) + " are free" + hint);
        const uint64_t whole = windowed ? sortc::window_span(piece_bytes, stream_max) : 0;
        if (!windowed) window_bytes = 0;
        else if (hook) window_bytes = sortc::window_span(piece_bytes, hook);
        else {
            // half of what is left goes to the window, the other half to the batch (~5 x its inflated bytes)
            const uint64_t avail = free_b - out_reserve - kMinBatch - min_arrays;
            window_bytes = std::min<uint64_t>(std::max<uint64_t>(avail / 2 / piece_bytes, 1) * piece_bytes, whole);
        }
        // The batch: 70 % of what the window and the encoder leave, a fifth of it inflated bytes (index_batch_bytes); the arrays take
        // per_record / 160 of the inflated bytes more, so the divisor grows by that.
        const uint64_t held = std::min<uint64_t>(window_bytes, whole);
        const uint64_t plain = index_batch_bytes(held + out_reserve);
        const bool hooked = getenv("SBX_INDEX_BATCH_BYTES") != nullptr;
        batch_u = std::min<uint64_t>(hooked ? plain : std::max<uint64_t>(64ull << 20, plain * 800 / (800 + per_record)), kWindowedBatchBytes);
    }
};

class StreamedOutput {
    hipStream_t s_;
    uint64_t hlen_, span_, w0_ = 0, at_ = 0;            // the window is [w0_, w0_ + span_); at_: bytes of the stream handed over so far
    sbx_stream_stats st_{};
    DevBuf<uint8_t> d_win_;
    DevBuf<unsigned long long> d_wacc_;
    DevBuf<uint64_t> d_group_sum_, d_dest_;
    DevBuf<uint32_t> d_len_;
    BgzfPieceCompressor comp_;
    BgzfPieceTimes bt_times_;
    OutputFile f_;
    EventTimer t_pack_;

    // the window [w0_, end) to the encoder: K21's counter against the record bytes that belong there
    void flush(uint64_t end) {
        unsigned long long wrote = 0;
        SBX_HIP(hipMemcpyAsync(&wrote, d_wacc_.p, sizeof wrote, hipMemcpyDeviceToHost, s_));
        SBX_HIP(hipMemsetAsync(d_wacc_.p, 0, sizeof wrote, s_));
        SBX_HIP(hipStreamSynchronize(s_));
        const uint64_t belong = streamc::window_record_bytes(w0_, w0_ + span_, hlen_, end);
        if (wrote != belong)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(wrote) + " record bytes arrived in bytes [" + std::to_string(w0_) + ", " +
                                         std::to_string(end) + ") of the output stream where " + std::to_string(belong) + " belong");
        comp_.run((size_t)(end - w0_), false, &bt_times_,
                  [&](uint8_t* d_in, size_t done, size_t bytes, hipStream_t ps) {
                      SBX_HIP(hipMemcpyAsync(d_in, d_win_.p + done, bytes, hipMemcpyDeviceToDevice, ps));
                  },
                  [&](const uint8_t* p, size_t k) { f_.write(p, k); });
        ++st_.n_windows;
        w0_ += span_;
    }
    // nb more bytes of the stream: fill(w0, w1) puts those of them that lie in [w0, w1) into the window; a window that is full goes out
    template <class Fill>
    void advance(uint64_t nb, Fill&& fill) {
        const uint64_t end = at_ + nb;
        while (nb) {
            fill(w0_, w0_ + span_);
            if (end < w0_ + span_) break;
            flush(w0_ + span_);
            if (end == w0_) break;
        }
        at_ = end;
    }

public:
    // `out` is armed as soon as the file exists and stays armed; the header is the first part of the stream.  stream_max: as for the budget.
    StreamedOutput(OutputGuard& out, const std::vector<uint8_t>& header, uint64_t stream_max, const StreamBudget& b, int level, hipStream_t s)
        // (a window is never larger than the stream in whole pieces)
        : StreamedOutput(out, header, std::min<uint64_t>(b.window_bytes, sortc::window_span(b.piece_bytes, stream_max)),
                         (uint32_t)std::min<uint64_t>(b.piece_blocks, std::max<uint64_t>(1, (stream_max + kBgzfPayload - 1) / kBgzfPayload)), level, s) {}
    // The same for a stream without a known bound (a pipe): a window of window_bytes (whole pieces, the caller's budget or the hook)
    // and an encoder for whole pieces of piece_blocks payloads.
    StreamedOutput(OutputGuard& out, const std::vector<uint8_t>& header, uint64_t window_bytes, uint32_t piece_blocks, int level, hipStream_t s)
        : s_(s), hlen_(header.size()), span_(window_bytes), d_win_((size_t)span_ + 64), d_wacc_(1), comp_(piece_blocks, level, true), f_(out) {
        st_.window_bytes = span_;
        SBX_HIP(hipMemsetAsync(d_wacc_.p, 0, sizeof(unsigned long long), s_));
        advance(hlen_, [&](uint64_t w0, uint64_t w1) {
            sortc::PieceClip c;
            if (sortc::clip_to_piece(0, hlen_, w0, w1, &c)) {
                SBX_HIP(hipMemcpyAsync(d_win_.p + c.dst, header.data() + c.src, c.len, hipMemcpyHostToDevice, s_));
                SBX_HIP(hipStreamSynchronize(s_));
            }
        });
    }
    // One described batch (a.U, a.desc, a.n, a.u_end, a.count, a.bin: the consumer's; the rest is filled in here) whose selected
    // records hold n_selected_bytes.  Returns when K21 has read what it needs of the batch: U may be overwritten.
    void add_batch(PackArgs a, uint64_t n_selected_bytes) {
        if (!a.n || !n_selected_bytes) return;
        d_group_sum_.ensure(pack_groups(a.n) + 2); d_dest_.ensure((size_t)a.n + 2); d_len_.ensure((size_t)a.n);
        a.stream_base = at_;
        a.group_sum = d_group_sum_.p; a.dest = d_dest_.p; a.len = d_len_.p;
        a.window = d_win_.p; a.acc = d_wacc_.p;
        t_pack_.start(s_);
        launch_pack_offsets(a, s_);
        t_pack_.stop(s_);
        double ms = t_pack_.ms();
        advance(n_selected_bytes, [&](uint64_t w0, uint64_t w1) {
            a.w0 = w0; a.w1 = w1;
            t_pack_.start(s_);
            launch_pack_records(a, s_);
            t_pack_.stop(s_);
            ms += t_pack_.ms();
            ++st_.n_pack_launches;
        });
        SBX_HIP(hipStreamSynchronize(s_));
        st_.ms_pack += ms;
    }
    // nb more bytes of the stream from a filler of the caller's: fill(window, w0, w1, counter) is called once for every window
    // [w0, w1) they touch, puts those of them that lie inside at window + (place - w0), in order on the stream, and adds their number
    // to *counter (device memory) -- the check of flush() holds for them as for K21's.  Returns when the last call of fill has.
    template <class Fill>
    void take(uint64_t nb, Fill&& fill) {
        double ms = 0;
        advance(nb, [&](uint64_t w0, uint64_t w1) {
            t_pack_.start(s_);
            fill(d_win_.p, w0, w1, d_wacc_.p);
            t_pack_.stop(s_);
            ms += t_pack_.ms();
            ++st_.n_pack_launches;
        });
        st_.ms_pack += ms;
    }
    // nb more bytes of the stream that lie in device memory at d_src: copies clipped to each window, counted like record bytes
    void take_device(const uint8_t* d_src, uint64_t nb) {
        const uint64_t from = at_;
        advance(nb, [&](uint64_t w0, uint64_t w1) {
            sortc::PieceClip c;
            if (!sortc::clip_to_piece(from, from + nb, w0, w1, &c)) return;
            unsigned long long count = 0;
            SBX_HIP(hipMemcpyAsync(d_win_.p + c.dst, d_src + c.src, c.len, hipMemcpyDeviceToDevice, s_));
            SBX_HIP(hipMemcpyAsync(&count, d_wacc_.p, sizeof count, hipMemcpyDeviceToHost, s_));
            SBX_HIP(hipStreamSynchronize(s_));
            count += c.len;
            SBX_HIP(hipMemcpyAsync(d_wacc_.p, &count, sizeof count, hipMemcpyHostToDevice, s_));
            SBX_HIP(hipStreamSynchronize(s_));
        });
    }
    // the last window, short; the EOF block
    void finish() {
        if (at_ > w0_) flush(at_);
        f_.finish(true);
        if (getenv("SBX_TIMING")) {
            fprintf(stderr, "[sbx] output: stream_bytes=%llu compressed_bytes=%llu n_pieces=%u\n", (unsigned long long)at_,
                    (unsigned long long)compressed_bytes(), bt_times_.n_pieces);
            fprintf(stderr, "[sbx] stream: n_windows=%u window_bytes=%llu n_pack_launches=%llu ms_pack=%.3f\n", st_.n_windows,
                    (unsigned long long)st_.window_bytes, (unsigned long long)st_.n_pack_launches, st_.ms_pack);
        }
    }
    uint64_t stream_bytes() const { return at_; }
    uint64_t compressed_bytes() const { return bt_times_.out_bytes + sizeof kEofBlock; }
    double ms_deflate() const { return bt_times_.ms_deflate + bt_times_.ms_pack; }
    const sbx_stream_stats& stats() const { return st_; }
};

}  // namespace sbx
