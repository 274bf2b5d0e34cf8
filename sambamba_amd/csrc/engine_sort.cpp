// engine_sort.cpp -- sbx_sort_bam: `sambamba sort` in coordinate order (sambamba/sort.d, default mode) on the device.
//
// One index-mode pass over the input (for_each_record_batch: K1 + K2 per batch, no sort order or index required); per batch K9a
// (sort.hip) writes key, store offset and length of every record that takes part, and the batch's record bytes are copied, device to
// device, behind those of the batches before: the resident record store, 1 x the inflated records of the file.  Then K9b sorts
// (key, record number) over the whole file, the lengths taken in sorted order are scanned into output offsets, and the sorted stream
// -- header bytes from the host, records gathered by K9c -- is produced in pieces of whole BGZF payloads that go straight into the
// deflate kernels (bgzf_compress_pieces) and, through pinned memory, to the file.  The sorted stream never exists as a whole.
//
// The scaffold of the entry point, the plan of the store, the copy into it and the output tail are engine_store.hpp, shared with
// sbx_markdup, sbx_merge_bam and sbx_view_bam.
// What does not fit the device next to one batch of the read pass is refused with SBX_ENOMEM (an out-of-core merge is not built).
#include "engine_store.hpp"
#include "sort_core.hpp"

extern "C" {

int sbx_sort_header_text(const char* text, size_t n, char* out, size_t cap, size_t* out_len) {
    if (!text && n) return SBX_EINVAL;
    std::string t;
    if (!sortc::sort_header_text(text ? text : "", n, &t, nullptr)) return SBX_EFORMAT;
    return copy_to_caller(t, out, cap, out_len);
}

int sbx_sort_bam(const char* in_path, const char* out_path, const sbx_filter* filter, int level, int with_index, int device,
                 sbx_sort_stats* stats, char* err, size_t errlen) {
    const int rc = run_entry(err, errlen, [&] {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        check_filter(filter);
        refuse_overwrite(in_path, out_path);
        const double w0 = wall_now();
        const bool use_filter = has_ops(filter);
        Standalone c = open_record_pass(in_path, device, filter, use_filter);
        OutputGuard out_file(out_path);
        const int32_t n_ref = (int32_t)c->hdr.refs.size();
        std::string text, why;
        if (!sortc::sort_header_text(c->hdr.text.data(), c->hdr.text.size(), &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        const std::vector<uint8_t> header = bam_header_bytes(text, c->hdr.refs);
        const uint64_t hlen = header.size();

        const StorePlan plan = plan_record_store(c.get(), hlen, 48, "sorting");
        const uint64_t u_total = plan.u_total, u_first = plan.u_first, store_bytes = plan.store_bytes, batch_u = plan.batch_u;
        hipStream_t s = c->stream.get();
        DevBuf<uint8_t> d_store((size_t)store_bytes + 64);
        DevBuf<uint64_t> d_key, d_off;
        DevBuf<uint32_t> d_len, d_group_count;
        DevBuf<uint64_t> d_group_base;
        DevBuf<unsigned long long> d_acc(kSortAccWords);
        {
            const unsigned long long init[kSortAccWords] = {0ull, ~0ull, 0ull, 0ull, 0ull};
            SBX_HIP(hipMemcpyAsync(d_acc.p, init, sizeof init, hipMemcpyHostToDevice, s));
            SBX_HIP(hipStreamSynchronize(s));
        }
        const double w1 = wall_now();

        // ---- the read pass ----
        sbx_sort_stats st{};
        EventTimer t_k;
        uint64_t n_in = 0, n_kept = 0, cur = u_first;
        uint32_t n_batches = 0;
        unsigned long long acc[kSortAccWords] = {0ull, ~0ull, 0ull, 0ull, 0ull};
        for_each_record_batch(c.get(), batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            const size_t want = (size_t)(n_kept + nrec + 2);
            grow_keeping(d_key, (size_t)n_kept, want, s);
            grow_keeping(d_off, (size_t)n_kept, want, s);
            grow_keeping(d_len, (size_t)n_kept, want, s);
            if (use_filter) { d_group_count.ensure(sort_keys_groups(nrec) + 4); d_group_base.ensure(sort_keys_groups(nrec) + 4); }
            t_k.start(s);
            copy_batch_to_store(c.get(), d_store.p, u_first, cur, base, next, s);
            SortKeysArgs a{};
            a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = next - base;
            a.n_ref = n_ref; a.key_n_ref = n_ref; a.use_filter = use_filter ? 1u : 0u;
            a.store_delta = (int64_t)base - (int64_t)u_first;
            a.out_base = n_kept;
            a.key = d_key.p; a.off = d_off.p; a.len = d_len.p; a.acc = d_acc.p;
            launch_sort_keys(a, d_group_count.p, d_group_base.p, s);
            t_k.stop(s);
            // (the next batch's K1 / K2 overwrite U and the descriptors: K9a and the copy end first)
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index; st.ms_keys += t_k.ms();
            n_in += nrec;
            n_kept = acc[kSortAccKept];
            cur = next;
            return acc[kSortAccBad] == 0;
        });
        if (acc[kSortAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kSortAccBad]));
        if (!use_filter && n_kept != n_in)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_kept) + " of " + std::to_string(n_in) + " records received a key");
        if (n_kept > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
        const uint64_t n = n_kept;
        c.reset();                                       // the batch buffers make room for the sort and the output pieces
        const double w2 = wall_now();

        // ---- K9b ----
        Stream stream;
        stream.create();
        s = stream.get();
        ResidentOrder order;
        sort_resident(d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
        // the keys are done with: one of their buffers holds the output offsets
        d_key.release();
        st.ms_sort = order.ms_sort;

        // ---- offsets, K9c + deflate, piece by piece ----
        const WrittenBam w = write_store_output(out_file, header, d_store.p, d_off.p, d_len, order.perm, n, order.key2.p, level,
                                                &acc[kSortAccBytes], "sorted records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = w.w_planned, w4 = wall_now();
        st.n_records_in = n_in; st.n_records_out = n;
        st.inflated_bytes = u_total; st.sorted_stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.key_bits = order.key_bits; st.n_sort_passes = order.n_passes; st.n_batches = n_batches;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (w4 - w0) * 1e3;
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] sort: n_records_in=%llu n_records_out=%llu inflated_bytes=%llu sorted_stream_bytes=%llu compressed_bytes=%llu "
                            "key_bits=%u n_sort_passes=%u n_batches=%u ms_inflate=%.2f ms_index=%.2f ms_keys=%.2f ms_sort=%.2f ms_gather=%.2f "
                            "ms_deflate=%.2f ms_total_wall=%.1f (open %.1f, read pass %.1f, sort %.1f, write %.1f)\n",
                    (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_out, (unsigned long long)st.inflated_bytes,
                    (unsigned long long)st.sorted_stream_bytes, (unsigned long long)st.compressed_bytes, st.key_bits, st.n_sort_passes, st.n_batches,
                    st.ms_inflate, st.ms_index, st.ms_keys, st.ms_sort, st.ms_gather, st.ms_deflate, st.ms_total_wall, (w1 - w0) * 1e3,
                    (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
        if (stats) *stats = st;
    });
    // (the index is a pass of its own and not part of the sort's figures)
    return rc != SBX_OK ? rc : index_written_bam(out_path, with_index, device, err, errlen);
}

}  // extern "C"
