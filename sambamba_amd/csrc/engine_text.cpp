// engine_text.cpp -- K6: the text of `depth base`, formatted on the device (format.hip) and copied out at once, left in device
// memory, or handed to a writer piece by piece.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "engine_ctx.hpp"

extern "C" {

// FormatArgs of a `depth base` run for rows of ref_id (the names blob travels on the stream first); beg / end are set by the caller
static FormatArgs format_args(sbx_ctx* c, uint32_t ref_id, double min_cov, double max_cov, int annotate, hipStream_t s) {
    const uint32_t S = c->n_samples_eff;
    // names blob: contig name, then the sample names ("*" when the header has no read groups, as the CLI prints)
    // (the blob on the device is kept while the next call asks for the same contig and sample names: a caller that formats a contig
    //  piece by piece does not pay two copies and a synchronisation per piece)
    std::string blob = c->hdr.refs[ref_id].name;
    std::vector<uint32_t> soff;
    for (uint32_t i = 0; i < S; ++i) {
        soff.push_back((uint32_t)blob.size());
        if (!c->combined && i < c->hdr.sample_names.size()) blob += c->hdr.sample_names[i];
    }
    soff.push_back((uint32_t)blob.size());
    if (!c->fmt_blob_on_device || blob != c->h_fmt_blob || soff != c->h_fmt_soff) {
        c->fmt_blob_on_device = false;
        c->h_fmt_blob = blob;
        c->h_fmt_soff = soff;
        c->d_fmt_names.ensure(c->h_fmt_blob.size() + 1);
        c->d_fmt_soff.ensure(c->h_fmt_soff.size());
        SBX_HIP(hipMemcpyAsync(c->d_fmt_names.p, c->h_fmt_blob.data(), c->h_fmt_blob.size(), hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_fmt_soff.p, c->h_fmt_soff.data(), c->h_fmt_soff.size() * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));         // (the host copies may be changed by the next call)
        c->fmt_blob_on_device = true;
    }
    FormatArgs a{};
    a.counters = c->d_counters.p;
    a.span = c->span_valid ? c->d_span.p : nullptr;
    a.slot_of = c->d_slot_of.p;
    a.tile_first = c->h_tile_base[ref_id];
    a.tile_end = c->h_tile_base[ref_id + 1];
    a.T = c->tile_pos;
    a.S = S;
    // COV is an integer: the reference's double comparisons (depth.d:538) become integer bounds
    if (!(max_cov >= 0) || !(min_cov <= max_cov)) { a.lo = 1; a.hi = 0; }
    else {
        a.lo = min_cov <= 0 ? 0 : (min_cov >= 1.8e19 ? ~0ull : (uint64_t)std::ceil(min_cov));
        a.hi = max_cov >= 1.8e19 ? ~0ull : (uint64_t)std::floor(max_cov);
    }
    a.annotate = annotate ? 1u : 0u;
    a.combined = c->combined ? 1u : 0u;
    a.zero_fill = min_cov <= 0 ? 1u : 0u;
    a.names = c->d_fmt_names.p;
    a.ref_name_len = (uint32_t)c->hdr.refs[ref_id].name.size();
    a.sample_off = c->d_fmt_soff.p;
    a.max_sample_len = 0;
    for (size_t i = 0; i + 1 < c->h_fmt_soff.size(); ++i) a.max_sample_len = std::max(a.max_sample_len, c->h_fmt_soff[i + 1] - c->h_fmt_soff[i]);
    return a;
}

// measure the rows of [a.beg, a.end): chunk offsets on the device, total bytes on the host (one synchronisation)
static uint64_t format_measure(sbx_ctx* c, const FormatArgs& a, uint32_t* n_chunks_out, hipStream_t s) {
    const uint32_t per = format_chunk_positions();
    const uint32_t n_chunks = (uint32_t)(((uint64_t)(a.end - a.beg) + per - 1) / per);
    c->d_fmt_len.ensure(n_chunks);
    c->d_fmt_off.ensure((size_t)n_chunks + 1);
    launch_format_measure(a, n_chunks, c->d_fmt_len.p, s);
    launch_count_scan(c->d_fmt_len.p, n_chunks, c->d_fmt_off.p, s);
    HostResults& R = results(c);
    SBX_HIP(hipMemcpyAsync(&R.last_state, c->d_fmt_off.p + n_chunks, 8, hipMemcpyDeviceToHost, s));
    SBX_HIP(hipStreamSynchronize(s));
    *n_chunks_out = n_chunks;
    return R.last_state;
}

static void check_base_run(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end, const char* who) {
    if (!c->have_run) throw Error(SBX_EINVAL, "sbx_run() has not been called");
    if (c->mode != SBX_MODE_BASE) throw Error(SBX_EINVAL, std::string(who) + " needs a `depth base` run");
    // (the layout of d_counters belongs to the run, not to the current mode setting: a compact run holds one word per position)
    if (c->compact_counters) throw Error(SBX_EINVAL, std::string(who) + ": the last run kept {bases, depth} per position, not the seven counters");
    if (ref_id >= c->hdr.refs.size() || beg > end) throw Error(SBX_EINVAL, "bad interval");
}

// the common head of sbx_format_base_rows(_device): the checks, the FormatArgs of [beg, end) and the size of its text
struct MeasuredRows {
    FormatArgs a{};
    uint32_t n_chunks = 0;
    uint64_t total = 0;
};

// false: an empty interval, nothing to format
static bool measure_rows(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov, int annotate,
                         const char* who, size_t* out_len, MeasuredRows* m) {
    check_base_run(c, ref_id, beg, end, who);
    hipStream_t s = c->stream.get();
    *out_len = 0;
    if (beg == end) return false;
    m->a = format_args(c, ref_id, min_cov, max_cov, annotate, s);
    m->a.beg = beg;
    m->a.end = end;
    m->total = format_measure(c, m->a, &m->n_chunks, s);
    *out_len = (size_t)m->total;
    return true;
}

int sbx_format_base_rows(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov, int annotate,
                         char* out, size_t cap, size_t* out_len) {
    return guarded(c, [&] {
        if (!c || !out_len) throw Error(SBX_EINVAL, "null argument");
        SBX_HIP(hipSetDevice(c->device));
        MeasuredRows m;
        if (!measure_rows(c, ref_id, beg, end, min_cov, max_cov, annotate, "sbx_format_base_rows", out_len, &m)) return;
        if (m.total > cap || (!out && m.total)) throw Error(SBX_ENOMEM, "output buffer too small for the formatted rows");
        if (!m.total) return;
        hipStream_t s = c->stream.get();
        c->d_fmt_text.ensure((size_t)m.total + 64);
        launch_format_write(m.a, m.n_chunks, c->d_fmt_off.p, c->d_fmt_text.p, s);
        SBX_HIP(hipMemcpyAsync(out, c->d_fmt_text.p, (size_t)m.total, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
    });
}

// The same text left in DEVICE memory (a consumer that compresses, checksums or ships it from there; bench.py's `device_text`): d_out
// is a device pointer of the context's device, or null to measure.
int sbx_format_base_rows_device(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov, int annotate,
                                void* d_out, size_t cap, size_t* out_len) {
    return guarded(c, [&] {
        if (!c || !out_len) throw Error(SBX_EINVAL, "null argument");
        MeasuredRows m;
        if (!measure_rows(c, ref_id, beg, end, min_cov, max_cov, annotate, "sbx_format_base_rows_device", out_len, &m)) return;
        if (!d_out && cap == 0) return;
        if (m.total > cap || !d_out) throw Error(SBX_ENOMEM, "output buffer too small for the formatted rows");
        if (!m.total) return;
        launch_format_write(m.a, m.n_chunks, c->d_fmt_off.p, (uint8_t*)d_out, c->stream.get());
        SBX_HIP(hipStreamSynchronize(c->stream.get()));
    });
}

// The same text handed to a writer piece by piece, in order: the device formats piece k + 1 while piece k travels to a
// pinned host buffer on the copy stream and the writer consumes piece k - 1 -- the D side passes the delegate that
// wraps its output File (sambamba/depth.d:1233-1234 flushes one in the reference).
int sbx_stream_base_rows(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end, double min_cov, double max_cov, int annotate,
                         sbx_write_fn write, void* user) {
    return guarded(c, [&] {
        if (!c || !write) throw Error(SBX_EINVAL, "null argument");
        check_base_run(c, ref_id, beg, end, "sbx_stream_base_rows");
        if (beg == end) return;
        struct Streaming {
            std::atomic<int>& n;
            explicit Streaming(std::atomic<int>& x) : n(x) { n.fetch_add(1); }
            ~Streaming() { n.fetch_sub(1); }
        } streaming_guard(c->text_streaming);
        hipStream_t s = c->stream.get(), ts = c->text_stream.get();
        FormatArgs a = format_args(c, ref_id, min_cov, max_cov, annotate, s);
        uint64_t piece = 2u << 20;                // positions per piece (~55 MB of text at one sample, 30x: the two pinned buffers
                                                  // of a context are allocated on first use, 15 ms each at this size)
        if (const char* e = getenv("SBX_STREAM_PIECE")) { const long v = atol(e); if (v >= 256) piece = (uint64_t)v; }      // (tests)
        size_t pending_len[2] = {0, 0};
        bool pending[2] = {false, false};
        auto drain = [&](int i) {
            if (!pending[i]) return;
            SBX_HIP(hipEventSynchronize(c->text_ev_copy[i].get()));
            pending[i] = false;
            if (pending_len[i] && write(user, (const char*)c->text_host[i].p, pending_len[i]) != 0)
                throw Error(SBX_EIO, "the output writer reported an error");
        };
        int k = 0;
        try {
        for (uint64_t p = beg; p < end; p += piece, k ^= 1) {
            a.beg = (uint32_t)p;
            a.end = (uint32_t)std::min<uint64_t>(end, p + piece);
            uint32_t n_chunks = 0;
            const uint64_t total = format_measure(c, a, &n_chunks, s);       // (synchronises the compute stream only)
            drain(k);                                                          // buffer k is free again once its piece is written
            if (total) {
                // (pieces differ in size by a few percent: a buffer that had to grow with every larger piece would be freed and
                //  allocated again and again, and hipFree waits for the whole device -- the copy of the previous piece included)
                if (c->d_fmt_text2[k].n < (size_t)total + 64) c->d_fmt_text2[k].alloc((size_t)total + (size_t)(total / 4) + (1u << 20));
                if (c->text_host[k].n < total) c->text_host[k].ensure((size_t)(total + total / 8 + (1u << 20)));
                launch_format_write(a, n_chunks, c->d_fmt_off.p, c->d_fmt_text2[k].p, s);
                SBX_HIP(hipEventRecord(c->text_ev_fmt[k].get(), s));
                SBX_HIP(hipStreamWaitEvent(ts, c->text_ev_fmt[k].get(), 0));
                SBX_HIP(hipMemcpyAsync(c->text_host[k].p, c->d_fmt_text2[k].p, (size_t)total, hipMemcpyDeviceToHost, ts));
                SBX_HIP(hipEventRecord(c->text_ev_copy[k].get(), ts));
                pending[k] = true;
                pending_len[k] = (size_t)total;
                // d_fmt_off / d_fmt_len are reused by the next measure: format_write of this piece must have read them
                SBX_HIP(hipEventSynchronize(c->text_ev_fmt[k].get()));
            }
            drain(k ^ 1);                                                      // the previous piece: copied while this one was formatted
        }
        drain(0);
        drain(1);
        } catch (...) {      // leave nothing in flight on the buffers the next call reuses
            (void)hipStreamSynchronize(ts);
            (void)hipStreamSynchronize(s);
            throw;
        }
    });
}

}  // extern "C"
