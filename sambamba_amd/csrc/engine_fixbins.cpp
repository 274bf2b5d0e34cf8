// engine_fixbins.cpp -- sbx_fixbins: `sambamba fixbins` (sambamba/fixbins.d) on the device.
//
// The shape is sbx_markdup's.  BinPass::step is the one batch step around K16b (bins.hip), called by both paths.  Resident: the batch
// is copied into the record store of engine_store.hpp, K16b notes offset and length of every record and stores
// reg2bin(pos, pos + basesCovered()) into the bin field of those that carry another value; the file is written in input order by the
// writer sort uses.  The header -- text and reference list -- is written as it was read: the reference adds no @PG line here.
//
// A file whose records do not fit the store (try_plan_record_store says so; or SBX_STREAM_WINDOW_BYTES) takes the streamed path
// (fixbins_streamed): no store; the same step computes the bins from the records in U and K21 (stream.hip) writes them while it
// copies the records into the staging window of engine_streamout.hpp.  The file is the same byte for byte.
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

// The read pass of both paths: the one batch step around K16b and what it keeps.
struct BinPass {
    sbx_ctx* c;
    hipStream_t s;
    PassBooks<kBinFixWords> books;
    DevBuf<uint64_t> d_off;         // resident: offset and length of every record in the store
    DevBuf<uint32_t> d_len, d_bin;  // streamed: the bins of one batch
    EventTimer t_k;
    double ms_bins = 0;
    uint64_t cur;                   // inflated offset of the file behind the batches so far

    BinPass(sbx_ctx* c_, uint64_t u_first, hipStream_t s_) : c(c_), s(s_), cur(u_first) { books.init(s); }
    // K16b over a batch of for_each_record_batch.  d_store: the resident record store -- the batch's bytes are copied behind those of
    // the batches before, inside the timed interval, the bins are stored there and off[] / len[] written -- or null: the bins go
    // to d_bin and nothing is stored into U (the streamed path).
    void step(uint64_t nrec, uint64_t base, uint64_t next, uint8_t* d_store, uint64_t u_first) {
        if (d_store) {
            const size_t want = (size_t)(books.n + nrec + 2);
            grow_keeping(d_off, (size_t)books.n, want, s);
            grow_keeping(d_len, (size_t)books.n, want, s);
        } else {
            d_bin.ensure((size_t)nrec + 2);
        }
        BinFixArgs a{};
        a.desc = c->d_desc.p; a.n = nrec; a.acc = books.d_acc.p;
        if (d_store) {
            a.store = d_store;
            a.store_delta = (int64_t)base - (int64_t)u_first;
            a.store_end = next - u_first;
            a.out_base = books.n;
            a.off = d_off.p; a.len = d_len.p;
        } else {
            a.store = const_cast<uint8_t*>(c->U());     // (with bin_out nothing is stored into it)
            a.store_end = next - base;
            a.bin_out = d_bin.p;
        }
        t_k.start(s);
        if (d_store) copy_batch_to_store(c, d_store, u_first, cur, base, next, s);
        launch_fix_bins(a, s);
        t_k.stop(s);
        // (the next batch's K1 / K2 overwrite U and the descriptors: K16b and the copy end first)
        books.read_back(c, nrec, s);
        ms_bins += t_k.ms();
        cur = next;
    }
    bool bad() const { return books.acc[kBinFixBad] != 0; }
    // after the pass: the refusals, then what the pass gives the stats
    void finish(const char* in_path, sbx_fixbins_stats* st) const {
        books.refuse_too_many();
        if (bad()) throw Error(SBX_EFORMAT, malformed_records_message(books.acc[kBinFixBad], in_path));
        st->n_records = books.n; st->n_bins_changed = books.acc[kBinFixChanged];
        st->ms_inflate = books.ms_inflate; st->ms_index = books.ms_index; st->ms_bins = ms_bins;
    }
};

void fixbins_streamed(Standalone& c, OutputGuard& out_file, const char* in_path, const std::vector<uint8_t>& header, uint64_t hook, int level,
                      double w0, sbx_fixbins_stats* stats, sbx_stream_stats* stream_stats) {
    const uint64_t u_total = c->blocks.out_off.back(), u_first = std::min<uint64_t>(c->hdr.first_record_off, u_total);
    const uint64_t stream_max = header.size() + (u_total - u_first);
    const StreamBudget budget(stream_max, hook, 20, "fixing the bins of", "20 bytes per record of it", "");
    hipStream_t s = c->stream.get();
    StreamedOutput out(out_file, header, stream_max, budget, level, s);
    BinPass bins(c.get(), u_first, s);
    const unsigned long long* acc = bins.books.acc;
    sbx_fixbins_stats st{};
    uint32_t n_batches = 0;
    for_each_record_batch(c.get(), budget.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
        if (!bins.books.admit(nrec)) return false;
        const unsigned long long bytes_before = acc[kBinFixBytes];
        bins.step(nrec, base, next, nullptr, 0);
        if (bins.bad()) return false;
        PackArgs p{};
        p.U = c->U(); p.desc = c->d_desc.p; p.n = nrec; p.u_end = next - base;
        p.bin = bins.d_bin.p;
        // (the next batch's K1 / K2 overwrite U and the descriptors: add_batch returns when K21 has read them)
        out.add_batch(p, acc[kBinFixBytes] - bytes_before);
        return true;
    });
    bins.finish(in_path, &st);
    out.finish();
    out_file.disarm();
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
        const std::optional<StorePlan> fits = hook ? std::nullopt : try_plan_record_store(c.get(), header.size(), 12, "fixing the bins of");
        if (!fits) { fixbins_streamed(c, out_file, in_path, header, hook, level, w0, stats, stream_stats); return; }
        const StorePlan& plan = *fits;
        const uint64_t u_first = plan.u_first;
        hipStream_t s = c->stream.get();
        DevBuf<uint8_t> d_store((size_t)plan.store_bytes + 64);
        BinPass bins(c.get(), u_first, s);
        const double w1 = wall_now();

        // ---- the read pass ----
        sbx_fixbins_stats st{};
        uint32_t n_batches = 0;
        for_each_record_batch(c.get(), plan.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            if (!bins.books.admit(nrec)) return false;
            bins.step(nrec, base, next, d_store.p, u_first);
            return !bins.bad();
        });
        bins.finish(in_path, &st);
        const uint64_t n = bins.books.n;
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
        const WrittenBam w = write_store_output(out_file, header, d_store.p, bins.d_off.p, bins.d_len, d_perm.p, n, d_out_off.p, level, &bins.books.acc[kBinFixBytes],
                                                "records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = wall_now();
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
