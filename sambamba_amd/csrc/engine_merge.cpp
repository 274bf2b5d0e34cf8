// engine_merge.cpp -- sbx_merge_bam: `sambamba merge` (sambamba/merge.d) for coordinate-sorted inputs on the device.
//
// The headers of the inputs are merged on the host (merge_core.hpp: SamHeaderMerger).  Then every input goes through the read pass of
// sbx_sort_bam in turn (for_each_record_batch: K1 + K2 per batch) and its records land in ONE resident record store, those of input
// k + 1 behind those of input k: rewritten by K11 (merge.hip) when the merged header gave the input other reference ids or renamed
// one of its @RG / @PG ids, copied device to device with K9a's keys otherwise.  The merge itself is K9b, the stable radix sort, over
// the keys of all records numbered input by input: records that compare equal come out lower input first, then in file order.  The
// writer is the one sort and markdup use (engine_store.hpp).  The reference merges sorted streams with a heap and trusts the headers;
// here the output is sorted whatever the records of the inputs say, and no .bai is needed when the dictionaries contradict one another.
//
// The two ways into the store do not check a record alike: K11 checks the fixed part and every aux field against block_size, the
// copy checks what sbx_sort_bam checks (block_size against the batch, ref_id against the dictionary, with a filter K2's verdict).
// A malformed aux field is SBX_EFORMAT in an input that is rewritten and copied as it is in one that is not (include/sbx_depth.h).
//
// Every input is opened twice: once for its header and size (the store is planned before the first record is read), once for its
// read pass.  One context is open at a time.
#include "engine_store.hpp"
#include "merge.hpp"
#include "merge_core.hpp"

namespace {

struct MergeInput {
    std::string text;               // header text, with @SQ lines made from the binary reference list when it has none
    uint64_t u_total = 0, u_first = 0;
    int32_t n_ref = 0;
    // what K11 needs
    std::vector<RenameEntry> entries;
    std::string blob;
    uint64_t grow_per_record = 0;   // the most bytes a record of this input can gain
    bool identity = true;
};

// The @SQ lines of a header text must be the binary reference list (the records speak the ids of the list, the merge works on the
// lines).  A text without @SQ lines gets them from the list, as BamReader does.
std::string text_with_sq_lines(const BamHeaderInfo& hdr, const std::string& path) {
    sortc::ParsedHeader ph;
    std::string why;
    if (!sortc::parse_header(hdr.text.data(), hdr.text.size(), &ph, &why)) throw Error(SBX_EFORMAT, "SAM header of " + path + ": " + why);
    std::string text = hdr.text;
    if (ph.sq.empty() && !hdr.refs.empty()) {
        if (!text.empty() && text.back() != '\n') text += '\n';
        for (const RefSeq& r : hdr.refs) text += "@SQ\tSN:" + r.name + "\tLN:" + std::to_string(r.length) + "\n";
        return text;
    }
    bool same = ph.sq.size() == hdr.refs.size();
    for (size_t k = 0; same && k < ph.sq.size(); ++k) same = ph.sq[k].id == hdr.refs[k].name;
    if (!same) throw Error(SBX_EFORMAT, "the @SQ lines of " + path + " are not its reference list");
    return text;
}

void add_renames(const mergec::IdMap& m, uint32_t kind, MergeInput* in) {
    uint64_t most = 0;
    for (const auto& e : m) {
        if (e.first == e.second) continue;
        RenameEntry x{};
        x.old_off = (uint32_t)in->blob.size(); x.old_len = (uint32_t)e.first.size();
        in->blob += e.first;
        x.new_off = (uint32_t)in->blob.size(); x.new_len = (uint32_t)e.second.size();
        in->blob += e.second;
        x.kind = kind;
        in->entries.push_back(x);
        if (e.second.size() > e.first.size()) most = std::max<uint64_t>(most, e.second.size() - e.first.size());
    }
    in->grow_per_record += most;     // (a record has at most one patch of a kind)
}

}  // namespace

extern "C" {

int sbx_merge_header_text(const char* const* texts, const size_t* lens, int n, char* out, size_t cap, size_t* out_len) {
    if (n < 1 || !texts || !lens) return SBX_EINVAL;
    std::vector<std::string> t;
    for (int k = 0; k < n; ++k) {
        if (!texts[k] && lens[k]) return SBX_EINVAL;
        t.emplace_back(texts[k] ? texts[k] : "", lens[k]);
    }
    mergec::MergedHeader m;
    std::string why;
    try {
        const int rc = mergec::merge_headers(t, &m, &why);
        return copy_to_caller(rc == SBX_OK ? m.text : why, out, cap, out_len, rc);
    } catch (const std::exception& e) {
        return copy_to_caller(e.what(), out, cap, out_len, SBX_EINVAL);
    }
}

int sbx_merge_bam(const char* out_path, const char* const* in_paths, int n_inputs, const sbx_filter* filter, int level, int with_index,
                  int device, sbx_merge_stats* stats, char* err, size_t errlen) {
    const int rc = run_entry(err, errlen, [&] {
        if (!out_path || !in_paths) throw Error(SBX_EINVAL, "null argument");
        if (n_inputs < 2) throw Error(SBX_EINVAL, "merging needs at least two input files");
        if (n_inputs > SBX_MERGE_MAX_INPUTS) throw Error(SBX_EINVAL, "more than " + std::to_string(SBX_MERGE_MAX_INPUTS) + " input files");
        check_level(level);
        check_filter(filter);
        for (int k = 0; k < n_inputs; ++k) {
            if (!in_paths[k]) throw Error(SBX_EINVAL, "null argument");
            refuse_overwrite(in_paths[k], out_path);
        }
        const double w0 = wall_now();
        const size_t n_in_files = (size_t)n_inputs;
        const bool use_filter = has_ops(filter);
        OutputGuard out_file(out_path);

        // ---- headers and sizes ----
        std::vector<MergeInput> in(n_in_files);
        std::vector<std::string> texts;
        uint64_t u_sum = 0;
        for (size_t k = 0; k < n_in_files; ++k) {
            Standalone c = open_standalone(in_paths[k], device);
            in[k].text = text_with_sq_lines(c->hdr, in_paths[k]);
            in[k].u_total = c->blocks.out_off.back();
            in[k].u_first = std::min<uint64_t>(c->hdr.first_record_off, in[k].u_total);
            in[k].n_ref = (int32_t)c->hdr.refs.size();
            u_sum += in[k].u_total;
            texts.push_back(in[k].text);
        }
        mergec::MergedHeader mh;
        {
            std::string why;
            const int rc = mergec::merge_headers(texts, &mh, &why);
            if (rc != SBX_OK) throw Error(rc, why);
        }
        const int32_t n_ref = (int32_t)mh.refs.size();
        const std::vector<uint8_t> header = bam_header_bytes(mh.text, mh.refs);
        const uint64_t hlen = header.size();
        const bool force_rewrite = getenv("SBX_MERGE_FORCE_REWRITE") && atoi(getenv("SBX_MERGE_FORCE_REWRITE")) != 0;

        // ---- the store ----
        // Capacity: the inflated record bytes of every input, plus a bound on what K11 adds to an input with renames.  A record gains
        // bytes only where an RG:Z / PG:Z value is replaced, at most once per kind, so at most g = (largest gain among the input's RG
        // renames) + (largest gain among its PG renames) per record; a record that holds such a tag is at least 40 bytes long
        // (block_size + 32 fixed bytes + tag, type and the NUL of the value), so an input of b bytes gains at most (b / 40 + 1) * g.
        uint64_t capacity = 0;
        for (size_t k = 0; k < n_in_files; ++k) {
            add_renames(mh.maps[k].rg, 0, &in[k]);
            add_renames(mh.maps[k].pg, 1, &in[k]);
            in[k].identity = mh.maps[k].identity();
            const uint64_t b = in[k].u_total - in[k].u_first;
            capacity += b + (b / 40 + 1) * in[k].grow_per_record;
        }
        const StorePlan plan = plan_store_bytes(capacity, hlen, 48, "merging", "the files do");     // (the device is the one the inputs were opened on)
        DevBuf<uint8_t> d_store((size_t)capacity + 64);
        DevBuf<uint64_t> d_key, d_off;
        DevBuf<uint32_t> d_len, d_group_count;
        DevBuf<uint64_t> d_group_base;
        DevBuf<unsigned long long> d_acc(kMergeAccWords);
        unsigned long long acc[kMergeAccWords] = {0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
        SBX_HIP(hipMemcpy(d_acc.p, acc, sizeof acc, hipMemcpyHostToDevice));
        // scratch of K11, per batch
        DevBuf<uint32_t> b_new_len, b_keep, b_patch_at, b_patch_entry;
        DevBuf<uint64_t> b_key, b_len_base, b_keep_base, b_tile_sum;
        const double w1 = wall_now();

        // ---- the read passes ----
        sbx_merge_stats st{};
        EventTimer t_k;
        uint64_t n_in = 0, n_kept = 0, store_at = 0, k11_new_bytes = 0;
        uint32_t n_batches = 0;
        bool too_many = false, store_full = false;
        for (size_t k = 0; k < n_in_files; ++k) {
            Standalone c = open_record_pass(in_paths[k], device, filter, use_filter);
            const bool fast = in[k].identity && !force_rewrite;
            hipStream_t s = c->stream.get();
            DevBuf<int32_t> d_ref_map(mh.maps[k].ref.size() + 1);
            DevBuf<RenameEntry> d_entries(in[k].entries.size() + 1);
            DevBuf<char> d_blob(in[k].blob.size() + 1);
            if (!fast) {
                if (!mh.maps[k].ref.empty()) SBX_HIP(hipMemcpy(d_ref_map.p, mh.maps[k].ref.data(), mh.maps[k].ref.size() * 4, hipMemcpyHostToDevice));
                if (!in[k].entries.empty()) {
                    SBX_HIP(hipMemcpy(d_entries.p, in[k].entries.data(), in[k].entries.size() * sizeof(RenameEntry), hipMemcpyHostToDevice));
                    SBX_HIP(hipMemcpy(d_blob.p, in[k].blob.data(), in[k].blob.size(), hipMemcpyHostToDevice));
                }
            }
            uint64_t cur = in[k].u_first;
            uint32_t nb = 0;
            for_each_record_batch(c.get(), plan.batch_u, &nb, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
                if (n_kept + nrec > 0xFFFFFFF0ull) { too_many = true; return false; }
                const size_t want = (size_t)(n_kept + nrec + 2);
                grow_keeping(d_key, (size_t)n_kept, want, s);
                grow_keeping(d_off, (size_t)n_kept, want, s);
                grow_keeping(d_len, (size_t)n_kept, want, s);
                if (fast) {
                    if (store_at + (next - cur) > capacity) { store_full = true; return false; }
                    if (use_filter) { d_group_count.ensure(sort_keys_groups(nrec) + 4); d_group_base.ensure(sort_keys_groups(nrec) + 4); }
                    t_k.start(s);
                    if (next > cur) SBX_HIP(hipMemcpyAsync(d_store.p + store_at, c->U() + (cur - base), next - cur, hipMemcpyDeviceToDevice, s));
                    SortKeysArgs a{};
                    a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = next - base;
                    a.n_ref = in[k].n_ref; a.key_n_ref = n_ref; a.use_filter = use_filter ? 1u : 0u;
                    a.store_delta = (int64_t)store_at + (int64_t)base - (int64_t)cur;
                    a.out_base = n_kept;
                    a.key = d_key.p; a.off = d_off.p; a.len = d_len.p; a.acc = d_acc.p;
                    launch_sort_keys(a, d_group_count.p, d_group_base.p, s);
                    t_k.stop(s);
                    SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipStreamSynchronize(s));
                    store_at += next - cur;
                } else {
                    const size_t m = (size_t)nrec + 2;
                    b_new_len.ensure(m); b_keep.ensure(m); b_key.ensure(m); b_patch_at.ensure(2 * m); b_patch_entry.ensure(2 * m);
                    b_len_base.ensure(m); b_keep_base.ensure(m); b_tile_sum.ensure(len_tiles(nrec) + 2);
                    MergeArgs a{};
                    a.U = c->U(); a.desc = c->d_desc.p; a.n = nrec; a.u_end = next - base;
                    a.n_ref_own = in[k].n_ref; a.n_ref_merged = n_ref; a.ref_map = d_ref_map.p;
                    a.table = RenameTable{d_entries.p, d_blob.p, (uint32_t)in[k].entries.size()};
                    a.use_filter = use_filter ? 1u : 0u;
                    a.b = MergeBatch{b_new_len.p, b_keep.p, b_key.p, b_patch_at.p, b_patch_entry.p, b_len_base.p, b_keep_base.p, b_tile_sum.p};
                    a.acc = d_acc.p;
                    a.store = d_store.p; a.store_at = store_at; a.out_base = n_kept;
                    a.key = d_key.p; a.off = d_off.p; a.len = d_len.p;
                    const unsigned long long bytes_before = acc[kSortAccBytes];
                    uint64_t batch_bytes = 0;
                    t_k.start(s);
                    launch_merge_describe(a, s);
                    SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
                    if (nrec) SBX_HIP(hipMemcpyAsync(&batch_bytes, b_len_base.p + nrec, 8, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipStreamSynchronize(s));
                    // the scanned size of the batch against what is left of the store, before a byte is written
                    if (!acc[kSortAccBad] && store_at + batch_bytes > capacity) store_full = true;
                    if (!acc[kSortAccBad] && !store_full) launch_merge_rewrite(a, s);
                    t_k.stop(s);
                    SBX_HIP(hipStreamSynchronize(s));
                    if (store_full) return false;
                    k11_new_bytes += acc[kSortAccBytes] - bytes_before;
                    store_at += batch_bytes;
                }
                // (the next batch's K1 / K2 overwrite U and the descriptors: the kernels above and the copy have ended)
                st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index; st.ms_rewrite += t_k.ms();
                n_in += nrec;
                n_kept = acc[kSortAccKept];
                cur = next;
                return acc[kSortAccBad] == 0;
            });
            n_batches += nb;
            c.reset();                                   // the batch buffers make room for the next input, the sort and the output pieces
            if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
            if (store_full) throw Error(SBX_ENOMEM, std::string("the record store is full at input ") + in_paths[k]);
            if (acc[kSortAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kSortAccBad], in_paths[k]));
        }
        if (!use_filter && n_kept != n_in)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_kept) + " of " + std::to_string(n_in) + " records received a key");
        const uint64_t n = n_kept;
        b_new_len.release(); b_keep.release(); b_key.release(); b_patch_at.release(); b_patch_entry.release();
        b_len_base.release(); b_keep_base.release(); b_tile_sum.release();
        const double w2 = wall_now();

        // ---- K9b: the merge ----
        Stream stream;
        stream.create();
        hipStream_t s = stream.get();
        ResidentOrder order;
        sort_resident(d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
        // the keys are done with: one of their buffers holds the output offsets
        d_key.release();
        st.ms_sort = order.ms_sort;

        // ---- offsets, K9c + deflate, piece by piece ----
        const WrittenBam w = write_store_output(out_file, header, d_store.p, d_off.p, d_len, order.perm, n, order.key2.p, level,
                                                &acc[kSortAccBytes], "merged records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = w.w_planned, w4 = wall_now();
        st.n_records_in = n_in; st.n_records_out = n;
        st.n_records_rewritten = acc[kMergeAccRewritten];
        st.bytes_grown = (int64_t)k11_new_bytes - (int64_t)acc[kMergeAccOldBytes];
        st.inflated_bytes = u_sum; st.merged_stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.n_inputs = (uint32_t)n_in_files; st.key_bits = order.key_bits; st.n_sort_passes = order.n_passes; st.n_batches = n_batches;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (w4 - w0) * 1e3;
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] merge: n_inputs=%u n_records_in=%llu n_records_out=%llu n_records_rewritten=%llu bytes_grown=%lld "
                            "inflated_bytes=%llu merged_stream_bytes=%llu compressed_bytes=%llu key_bits=%u n_sort_passes=%u n_batches=%u "
                            "ms_inflate=%.2f ms_index=%.2f ms_rewrite=%.2f ms_sort=%.2f ms_gather=%.2f ms_deflate=%.2f ms_total_wall=%.1f "
                            "(headers %.1f, read passes %.1f, sort %.1f, write %.1f)\n",
                    st.n_inputs, (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_out,
                    (unsigned long long)st.n_records_rewritten, (long long)st.bytes_grown, (unsigned long long)st.inflated_bytes,
                    (unsigned long long)st.merged_stream_bytes, (unsigned long long)st.compressed_bytes, st.key_bits, st.n_sort_passes, st.n_batches,
                    st.ms_inflate, st.ms_index, st.ms_rewrite, st.ms_sort, st.ms_gather, st.ms_deflate, st.ms_total_wall, (w1 - w0) * 1e3,
                    (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
        if (stats) *stats = st;
    });
    // (the index is a pass of its own and not part of the merge's figures)
    return rc != SBX_OK ? rc : index_written_bam(out_path, with_index, device, err, errlen);
}

}  // extern "C"
