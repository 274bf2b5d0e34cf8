// engine_fixbins.cpp -- sbx_fixbins: `sambamba fixbins` (sambamba/fixbins.d) on the device.
//
// The shape is sbx_markdup's: the read pass of engine_store.hpp copies every batch of records into the resident record store; per
// batch K16b (bins.hip) notes offset and length of every record and stores reg2bin(pos, pos + basesCovered()) into the bin field of
// those that carry another value; the file is written in input order by the writer sort uses.  The header -- text and reference list
// -- is written as it was read: the reference adds no @PG line here.
//
// A file whose records do not fit the store (or SBX_STREAM_WINDOW_BYTES) takes the streamed path (fixbins_streamed): no store; per
// batch K16b computes the bins from the records in U and K21 (stream.hip) writes them while it copies the records into the staging
// window of engine_streamout.hpp.  The file is the same byte for byte.
#include "bins.hpp"
#include "engine_streamout.hpp"

namespace {

// the `[sbx] fixbins:` line of SBX_TIMING=1; tail: what the path adds behind the fields of the stats
void print_timing(const sbx_fixbins_stats& st, const char* tail) {
    if (!getenv("SBX_TIMING")) return;
    fprintf(stderr, "[sbx] fixbins: n_records=%llu n_bins_changed=%llu inflated_bytes=%llu stream_bytes=%llu compressed_bytes=%llu "
                    "n_batches=%u ms_inflate=%.2f ms_index=%.2f ms_bins=%.3f ms_gather=%.2f ms_deflate=%.2f ms_total_wall=%.1f%s\n",
            (unsigned long long)st.n_records, (unsigned long long)st.n_bins_changed, (unsigned long long)st.inflated_bytes,
            (unsigned long long)st.stream_bytes, (unsigned long long)st.compressed_bytes, st.n_batches, st.ms_inflate, st.ms_index,
            st.ms_bins, st.ms_gather, st.ms_deflate, st.ms_total_wall, tail);
}

void fixbins_streamed(Standalone& c, OutputGuard& out_file, const char* in_path, const std::vector<uint8_t>& header, uint64_t hook, int level,
                      double w0, sbx_fixbins_stats* stats, sbx_stream_stats* stream_stats) {
    const uint64_t u_total = c->blocks.out_off.back(), u_first = std::min<uint64_t>(c->hdr.first_record_off, u_total);
    const uint64_t stream_max = header.size() + (u_total - u_first);
    const StreamBudget budget(stream_max, hook, 20, "fixing the bins of", "20 bytes per record of it", "");
    hipStream_t s = c->stream.get();
    StreamedOutput out(out_file, header, stream_max, budget, level, s);
    DevBuf<uint32_t> d_bin;
    DevBuf<unsigned long long> d_acc(kBinFixWords);
    SBX_HIP(hipMemsetAsync(d_acc.p, 0, kBinFixWords * sizeof(unsigned long long), s));
    SBX_HIP(hipStreamSynchronize(s));
    sbx_fixbins_stats st{};
    EventTimer t_k;
    uint64_t n = 0;
    uint32_t n_batches = 0;
    bool too_many = false;
    unsigned long long acc[kBinFixWords] = {0};
    for_each_record_batch(c.get(), budget.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
        if (n + nrec > 0xFFFFFFF0ull) { too_many = true; return false; }
        d_bin.ensure((size_t)nrec + 2);
        const unsigned long long bytes_before = acc[kBinFixBytes];
        t_k.start(s);
        BinFixArgs a{};
        a.store = const_cast<uint8_t*>(c->U()); a.desc = c->d_desc.p; a.n = nrec;      // (with bin_out nothing is stored into it)
        a.store_delta = 0;
        a.store_end = next - base;
        a.acc = d_acc.p;
        a.bin_out = d_bin.p;
        launch_fix_bins(a, s);
        t_k.stop(s);
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index; st.ms_bins += t_k.ms();
        n += nrec;
        if (acc[kBinFixBad]) return false;
        PackArgs p{};
        p.U = c->U(); p.desc = c->d_desc.p; p.n = nrec; p.u_end = next - base;
        p.bin = d_bin.p;
        // (the next batch's K1 / K2 overwrite U and the descriptors: add_batch returns when K21 has read them)
        out.add_batch(p, acc[kBinFixBytes] - bytes_before);
        return true;
    });
    if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
    if (acc[kBinFixBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kBinFixBad], in_path));
    out.finish();
    out_file.disarm();
    st.n_records = n; st.n_bins_changed = acc[kBinFixChanged];
    st.inflated_bytes = u_total; st.stream_bytes = out.stream_bytes(); st.compressed_bytes = out.compressed_bytes();
    st.n_batches = n_batches;
    st.ms_deflate = out.ms_deflate();
    st.ms_total_wall = (wall_now() - w0) * 1e3;
    print_timing(st, "");
    if (stats) *stats = st;
    if (stream_stats) *stream_stats = out.stats();
}

}  // namespace

extern "C" {

int sbx_fixbins_run(const char* in_path, const char* out_path, int level, int device, sbx_fixbins_stats* stats, sbx_stream_stats* stream_stats,
                    char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        refuse_overwrite(in_path, out_path);
        if (stream_stats) *stream_stats = sbx_stream_stats{};
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, nullptr, false);
        OutputGuard out_file(out_path);
        const std::vector<uint8_t> header = bam_header_bytes(c->hdr.text, c->hdr.refs);
        // the resident store, unless it does not fit or the hook asks for the stream
        const uint64_t hook = stream_window_hook();
        StorePlan plan{};
        bool streamed = hook != 0;
        if (!streamed) {
            try { plan = plan_record_store(c.get(), header.size(), 12, "fixing the bins of"); }
            catch (const Error& e) { if (e.code != SBX_ENOMEM) throw; streamed = true; }
        }
        if (streamed) { fixbins_streamed(c, out_file, in_path, header, hook, level, w0, stats, stream_stats); return; }
        const uint64_t u_first = plan.u_first;
        hipStream_t s = c->stream.get();
        DevBuf<uint8_t> d_store((size_t)plan.store_bytes + 64);
        DevBuf<uint64_t> d_off;
        DevBuf<uint32_t> d_len;
        DevBuf<unsigned long long> d_acc(kBinFixWords);
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, kBinFixWords * sizeof(unsigned long long), s));
        SBX_HIP(hipStreamSynchronize(s));
        const double w1 = wall_now();

        // ---- the read pass ----
        sbx_fixbins_stats st{};
        EventTimer t_k;
        uint64_t n = 0, cur = u_first;
        uint32_t n_batches = 0;
        bool too_many = false;
        unsigned long long acc[kBinFixWords] = {0};
        for_each_record_batch(c.get(), plan.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            if (n + nrec > 0xFFFFFFF0ull) { too_many = true; return false; }
            const size_t want = (size_t)(n + nrec + 2);
            grow_keeping(d_off, (size_t)n, want, s);
            grow_keeping(d_len, (size_t)n, want, s);
            t_k.start(s);
            copy_batch_to_store(c.get(), d_store.p, u_first, cur, base, next, s);
            BinFixArgs a{};
            a.store = d_store.p; a.desc = c->d_desc.p; a.n = nrec;
            a.store_delta = (int64_t)base - (int64_t)u_first;
            a.store_end = next - u_first;
            a.out_base = n;
            a.off = d_off.p; a.len = d_len.p; a.acc = d_acc.p;
            launch_fix_bins(a, s);
            t_k.stop(s);
            // (the next batch's K1 / K2 overwrite U and the descriptors: K16b and the copy end first)
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index; st.ms_bins += t_k.ms();
            n += nrec;
            cur = next;
            return acc[kBinFixBad] == 0;
        });
        if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
        if (acc[kBinFixBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kBinFixBad], in_path));
        const uint64_t u_total = plan.u_total;
        c.reset();                                       // the batch buffers make room for the output pieces
        const double w2 = wall_now();

        // ---- the output: the records of the store in their order ----
        Stream stream;
        stream.create();
        s = stream.get();
        DevBuf<uint32_t> d_perm((size_t)n + 2);
        launch_iota(d_perm.p, n, s);
        DevBuf<uint64_t> d_out_off((size_t)n + 2);
        const WrittenBam w = write_store_output(out_file, header, d_store.p, d_off.p, d_len, d_perm.p, n, d_out_off.p, level, &acc[kBinFixBytes],
                                                "records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = wall_now();
        st.n_records = n; st.n_bins_changed = acc[kBinFixChanged];
        st.inflated_bytes = u_total; st.stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.n_batches = n_batches;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (w3 - w0) * 1e3;
        char phases[96];
        snprintf(phases, sizeof phases, " (open %.1f, read pass %.1f, write %.1f)", (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3);
        print_timing(st, phases);
        if (stats) *stats = st;
    });
}

int sbx_fixbins(const char* in_path, const char* out_path, int level, int device, sbx_fixbins_stats* stats, char* err, size_t errlen) {
    return sbx_fixbins_run(in_path, out_path, level, device, stats, nullptr, err, errlen);
}

}  // extern "C"
