// engine_subsample.cpp -- sbx_subsample: `sambamba subsample --type fasthash --max-cov N [-r]` (sambamba/subsample.d, which is
// unfinished: DESIGN.md section 8 defines what this computes) on the device.
//
// The coverage a record is judged by is that of the WHOLE file, so the file is read twice: the first pass of for_each_record_batch
// marks the span ends of every counted record in the coverage array D (K22a, subsample.hip), K22b scans D in place, and the second
// pass over the same context judges every record against D (K22c) and hands the batch to the streamed writer of
// engine_streamout.hpp -- with -r K21 leaves the dropped records out, without it K21 writes flag | 0x200 into bytes 18 .. 19 of a
// dropped record while it copies it.  There is no record store: D is what stays resident, and StreamBudget is taken AFTER D is
// allocated, so the window and the read batch share what D leaves.  (A variant that keeps the records of a small file resident and
// reads it once is a follow-up.)
#include "engine_streamout.hpp"
#include "markdup_core.hpp"
#include "subsample.hpp"

namespace {

void print_timing(const sbx_subsample_stats& st) {
    if (!getenv("SBX_TIMING")) return;
    fprintf(stderr, "[sbx] subsample: n_records=%llu n_counted=%llu n_over=%llu n_dropped=%llu n_written=%llu max_cov_seen=%llu "
                    "cov_array_bytes=%llu inflated_bytes=%llu stream_bytes=%llu compressed_bytes=%llu n_batches=%u ms_inflate=%.2f "
                    "ms_index=%.2f ms_mark=%.3f ms_scan=%.3f ms_verdict=%.3f ms_deflate=%.2f ms_total_wall=%.1f\n",
            (unsigned long long)st.n_records, (unsigned long long)st.n_counted, (unsigned long long)st.n_over,
            (unsigned long long)st.n_dropped, (unsigned long long)st.n_written, (unsigned long long)st.max_cov_seen,
            (unsigned long long)st.cov_array_bytes, (unsigned long long)st.inflated_bytes, (unsigned long long)st.stream_bytes,
            (unsigned long long)st.compressed_bytes, st.n_batches, st.ms_inflate, st.ms_index, st.ms_mark, st.ms_scan, st.ms_verdict,
            st.ms_deflate, st.ms_total_wall);
}

}  // namespace

extern "C" {

int sbx_subsample(const char* in_path, const char* out_path, int max_cov, int remove, int level, int with_index,
                  const char* pg_command_line, int device, sbx_subsample_stats* stats, sbx_stream_stats* stream_stats, char* err,
                  size_t errlen) {
    const int rc = run_entry(err, errlen, [&] {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        if (max_cov <= 0) throw Error(SBX_EINVAL, "Maximum coverage not set");
        check_level(level);
        refuse_overwrite(in_path, out_path);
        if (stream_stats) *stream_stats = sbx_stream_stats{};
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, nullptr, false);
        OutputGuard out_file(out_path);
        std::string text, why;
        if (!mdc::markdup_header_text(c->hdr.text.data(), c->hdr.text.size(), pg_command_line, &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        const std::vector<uint8_t> header = bam_header_bytes(text, c->hdr.refs);
        hipStream_t s = c->stream.get();

        // ---- the coverage array: one slot per position of every reference and one more per reference, in whole tiles of the scan ----
        const int32_t n_ref = (int32_t)c->hdr.refs.size();
        std::vector<int32_t> ln((size_t)n_ref);
        for (int32_t r = 0; r < n_ref; ++r) ln[(size_t)r] = c->hdr.refs[(size_t)r].length;
        const std::vector<uint64_t> base = subc::slot_bases(ln.data(), (size_t)n_ref);
        const uint64_t n_tiles = subc::cov_tiles(base.back());
        const uint64_t cov_bytes = n_tiles * subc::kCovTile * sizeof(uint32_t);
        const std::string share = "the coverage array takes " + std::to_string(cov_bytes) + " bytes of it, 4 per reference position";
        size_t free_b = 0, total_b = 0;
        SBX_HIP(hipMemGetInfo(&free_b, &total_b));
        if (cov_bytes + StreamBudget::kMinBatch > free_b)
            throw Error(SBX_ENOMEM, std::string("the coverage of ") + in_path + " does not fit the device: capping it needs more than " +
                                        std::to_string(cov_bytes + StreamBudget::kMinBatch) + " bytes of device memory (" + share + "), " +
                                        std::to_string(free_b) + " are free");
        DevBuf<uint32_t> d_cov((size_t)(n_tiles * subc::kCovTile) + 4);
        DevBuf<uint64_t> d_base(base.size()), d_tile_sum((size_t)n_tiles + 2);
        DevBuf<unsigned long long> d_acc(kCovWords);
        SBX_HIP(hipMemsetAsync(d_cov.p, 0, d_cov.bytes(), s));
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, kCovWords * sizeof(unsigned long long), s));
        SBX_HIP(hipMemcpyAsync(d_base.p, base.data(), base.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));

        // ---- what D leaves: one read batch, K22c's word and K21's arrays per record, the encoder, one window ----
        const uint64_t u_total = c->blocks.out_off.back(), u_first = std::min<uint64_t>(c->hdr.first_record_off, u_total);
        const uint64_t stream_max = header.size() + (u_total - u_first);
        const uint64_t hook = stream_window_hook();
        const std::string hint = "; " + share;
        const StreamBudget budget(stream_max, hook, 20, "capping the coverage of", "20 bytes per record of it", hint.c_str());

        sbx_subsample_stats st{};
        st.cov_array_bytes = cov_bytes;
        EventTimer t_k;
        unsigned long long acc[kCovWords] = {0};
        CovArgs a{};
        a.base = d_base.p; a.n_ref = n_ref; a.D = d_cov.p; a.acc = d_acc.p;
        a.max_cov = (uint32_t)max_cov;
        auto run_kernel = [&](uint64_t nrec, uint64_t base_u, uint64_t next, bool verdict, double* ms) {
            a.U = c->U(); a.desc = c->d_desc.p; a.n = nrec; a.u_end = next - base_u;
            t_k.start(s);
            if (verdict) launch_cov_verdict(a, s);
            else launch_cov_mark(a, s);
            t_k.stop(s);
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index;
            *ms += t_k.ms();
        };

        // ---- pass 1: K22a ----
        uint64_t n = 0;
        uint32_t n_batches = 0;
        bool too_many = false;
        for_each_record_batch(c.get(), budget.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base_u, uint64_t next) -> bool {
            if (n + nrec > 0xFFFFFFF0ull) { too_many = true; return false; }
            run_kernel(nrec, base_u, next, false, &st.ms_mark);
            n += nrec;
            return acc[kCovBad] == 0;
        });
        if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
        if (acc[kCovBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kCovBad], in_path));
        st.n_batches = n_batches;

        // ---- K22b ----
        t_k.start(s);
        launch_cov_scan(d_cov.p, n_tiles, d_tile_sum.p, s);
        t_k.stop(s);
        SBX_HIP(hipStreamSynchronize(s));
        st.ms_scan = t_k.ms();

        // ---- pass 2: K22c, K21 ----
        StreamedOutput out(out_file, header, stream_max, budget, level, s);
        DevBuf<uint32_t> d_word;            // count[] with -r, patch[] without
        uint64_t n2 = 0;
        for_each_record_batch(c.get(), budget.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base_u, uint64_t next) -> bool {
            d_word.ensure((size_t)nrec + 2);
            a.count = remove ? d_word.p : nullptr;
            a.patch = remove ? nullptr : d_word.p;
            const unsigned long long bytes_before = acc[kCovBytes];
            run_kernel(nrec, base_u, next, true, &st.ms_verdict);
            n2 += nrec;
            if (acc[kCovBad]) return false;
            PackArgs p{};
            p.U = c->U(); p.desc = c->d_desc.p; p.n = nrec; p.u_end = next - base_u;
            p.count = a.count;
            p.bin = a.patch;
            p.patch_off = streamc::kFlagOffset;
            // (the next batch's K1 / K2 overwrite U and the descriptors: add_batch returns when K21 has read them)
            out.add_batch(p, acc[kCovBytes] - bytes_before);
            return true;
        });
        if (acc[kCovBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kCovBad], in_path));
        if (n2 != n) throw Error(SBX_EIO, "the input changed between the two read passes (" + std::to_string(n) + " records, then " + std::to_string(n2) + ")");
        out.finish();
        out_file.disarm();
        st.n_batches += n_batches;
        st.n_records = n; st.n_counted = acc[kCovCounted]; st.n_over = acc[kCovOver]; st.n_dropped = acc[kCovDropped];
        st.n_written = remove ? n - acc[kCovDropped] : n;
        st.max_cov_seen = acc[kCovMaxSeen];
        st.inflated_bytes = u_total; st.stream_bytes = out.stream_bytes(); st.compressed_bytes = out.compressed_bytes();
        st.ms_deflate = out.ms_deflate();
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        print_timing(st);
        if (stats) *stats = st;
        if (stream_stats) *stream_stats = out.stats();
    });
    // (the index is a pass of its own and not part of the figures)
    return rc != SBX_OK ? rc : index_written_bam(out_path, with_index, device, err, errlen);
}

}  // extern "C"
