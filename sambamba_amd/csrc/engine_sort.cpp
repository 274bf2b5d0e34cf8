// engine_sort.cpp -- sbx_sort_bam: `sambamba sort` in coordinate order (sambamba/sort.d, default mode) on the device.
//
// One index-mode pass over the input (for_each_record_batch: K1 + K2 per batch, no sort order or index required); per batch K9a
// (sort.hip) writes key, store offset and length of every record that takes part, and the batch's record bytes are copied, device to
// device, behind those of the batches before: the resident record store, 1 x the inflated records of the file.  Then K9b sorts
// (key, record number) over the whole file, the lengths taken in sorted order are scanned into output offsets, and the sorted stream
// -- header bytes from the host, records gathered by K9c -- is produced in pieces of whole BGZF payloads that go straight into the
// deflate kernels (bgzf_compress_pieces) and, through pinned memory, to the file.  The sorted stream never exists as a whole.
//
// The plan of the store, the copy into it and the writer are engine_store.hpp, shared with sbx_markdup.
// What does not fit the device next to one batch of the read pass is refused with SBX_ENOMEM (an out-of-core merge is not built).
#include "engine_store.hpp"
#include "sort_core.hpp"

extern "C" {

int sbx_sort_header_text(const char* text, size_t n, char* out, size_t cap, size_t* out_len) {
    if (!text && n) return SBX_EINVAL;
    std::string t;
    if (!sortc::sort_header_text(text ? text : "", n, &t, nullptr)) return SBX_EFORMAT;
    if (out_len) *out_len = t.size();
    if (!out || t.size() + 1 > cap) return SBX_ENOMEM;
    memcpy(out, t.data(), t.size());
    out[t.size()] = 0;
    return SBX_OK;
}

int sbx_sort_bam(const char* in_path, const char* out_path, const sbx_filter* filter, int level, int with_index, int device,
                 sbx_sort_stats* stats, char* err, size_t errlen) {
    sbx_ctx* c = nullptr;
    bool out_created = false;
    auto fail = [&](int code, const std::string& m) {
        set_err(err, errlen, m);
        if (c) sbx_close(c);
        if (out_created) unlink(out_path);
        return code;
    };
    try {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        if (level < -1 || level > 9) throw Error(SBX_EINVAL, "compression level must be -1 (default) or 0 .. 9");
        if (filter && (filter->n_ops < 0 || filter->n_ops > SBX_FILTER_MAX_OPS)) throw Error(SBX_EINVAL, "malformed filter");
        if (same_file(in_path, out_path)) throw Error(SBX_EINVAL, std::string("the output would overwrite the input ") + in_path);
        const double w0 = wall_now();
        const char* one[1] = {in_path};
        char e2[512] = {0};
        c = sbx_open(one, 1, device, e2, sizeof e2);
        if (!c) throw Error(t_open_code != SBX_OK ? t_open_code : SBX_EIO, e2);
        c->index_mode = true;                            // every record is described; no sort order, index or read group is required
        memset(&c->filter, 0, sizeof c->filter);
        if (filter && filter->n_ops > 0) { c->filter = *filter; c->filter_every = true; }
        c->mode = SBX_MODE_BASE;
        c->fix_mate = false;
        const bool use_filter = c->filter_every;
        const int32_t n_ref = (int32_t)c->hdr.refs.size();
        std::string text, why;
        if (!sortc::sort_header_text(c->hdr.text.data(), c->hdr.text.size(), &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        const std::vector<uint8_t> header = bam_header_bytes(text, c->hdr.refs);
        const uint64_t hlen = header.size();

        const StorePlan plan = plan_record_store(c, hlen, 48, "sorting");
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
        for_each_record_batch(c, batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            const size_t want = (size_t)(n_kept + nrec + 2);
            grow_keeping(d_key, (size_t)n_kept, want, s);
            grow_keeping(d_off, (size_t)n_kept, want, s);
            grow_keeping(d_len, (size_t)n_kept, want, s);
            if (use_filter) { d_group_count.ensure(sort_keys_groups(nrec) + 4); d_group_base.ensure(sort_keys_groups(nrec) + 4); }
            t_k.start(s);
            copy_batch_to_store(c, d_store.p, u_first, cur, base, next, s);
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
        if (acc[kSortAccBad])
            throw Error(SBX_EFORMAT, "malformed BAM record (" + std::to_string(acc[kSortAccBad]) + " records whose reference id is out of range or "
                                     "whose lengths are inconsistent)");
        if (!use_filter && n_kept != n_in)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_kept) + " of " + std::to_string(n_in) + " records received a key");
        if (n_kept > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
        const uint64_t n = n_kept;
        sbx_close(c);                                    // the batch buffers make room for the sort and the output pieces
        c = nullptr;
        const double w2 = wall_now();

        // ---- K9b ----
        Stream stream;
        stream.create();
        s = stream.get();
        ResidentOrder order;
        sort_resident(d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
        const uint32_t* d_perm = order.perm;
        const uint32_t key_bits = order.key_bits, n_passes = order.n_passes;
        // the keys are done with: one of their buffers holds the output offsets
        uint64_t* d_out_off = order.key2.p;
        d_key.release();
        const OutputPlan out = plan_output(d_len.p, d_perm, n, hlen, d_out_off, s, &st.ms_gather);
        const uint64_t total = out.total;
        st.ms_sort = order.ms_sort;
        if (total != hlen + acc[kSortAccBytes]) throw Error(SBX_EFORMAT, "internal error: the offsets of the sorted records do not add up");
        d_len.release();
        const double w3 = wall_now();

        // ---- K9c + deflate, piece by piece ----
        BgzfPieceTimes bt_times;
        write_permuted_bam(out_path, header, out, d_store.p, d_off.p, d_perm, d_out_off, n, level, &out_created, &st.ms_gather, &bt_times);
        const double w4 = wall_now();
        st.n_records_in = n_in; st.n_records_out = n;
        st.inflated_bytes = u_total; st.sorted_stream_bytes = total; st.compressed_bytes = bt_times.out_bytes + 28;
        st.key_bits = key_bits; st.n_sort_passes = n_passes; st.n_batches = n_batches;
        st.ms_deflate = bt_times.ms_deflate + bt_times.ms_pack;
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
    } catch (const Error& e) {
        return fail(e.code, e.what());
    } catch (const std::exception& e) {
        return fail(SBX_EINVAL, e.what());
    }
    if (with_index) {
        const int rc = sbx_build_index(out_path, (std::string(out_path) + ".bai").c_str(), device, err, errlen);
        if (rc != SBX_OK) return rc;          // (the index is a pass of its own and not part of the sort's figures)
    }
    return SBX_OK;
}

}  // extern "C"
