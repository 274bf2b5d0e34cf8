// engine_markdup.cpp -- sbx_markdup: `sambamba markdup` (sambamba/markdup.d) on the device.
//
// The read pass is that of sbx_sort_bam (engine_store.hpp: every batch of records is copied into the resident record store); per
// batch K10a (markdup.hip) describes every record -- class, position key, score, name + RG hash.  Then, over the whole file: the
// pairable records are sorted by hash and paired inside the runs (K10b); the pairs are sorted by their three key words, the single
// ends and one marker per pair end by their two (K10c: LSD over the words with K9b's passes, a key gather between the words, digits
// that do not vary skipped); "not the first of its group" marks the duplicates; K10d patches the flags in the store; the file is
// written in input order -- with -r without the marked records -- by the writer sort uses.
#include "engine_store.hpp"
#include "markdup.hpp"
#include "markdup_core.hpp"

namespace {

// (index, key) buffers of the radix sort and the sort of indices by one 64-bit word of their entries
struct WordSorter {
    DevBuf<uint64_t> key[2];
    DevBuf<uint32_t> val[2];
    DevBuf<uint32_t> hist;
    DevBuf<uint64_t> hist_base;
    int at = 0;
    uint32_t passes = 0;
    void reserve(uint64_t n) {
        for (int k = 0; k < 2; ++k) { key[k].ensure((size_t)n + 2); val[k].ensure((size_t)n + 2); }
        hist.ensure(radix_hist_entries(n) + 4);
        hist_base.ensure(radix_hist_entries(n) + 4);
    }
    uint32_t* idx() { return val[at].p; }
    const uint64_t* keys() { return key[at].p; }
    // idx()[0, n) are indices into d_word: sorts them by d_word[index], stable.  keys() holds the words in sorted order afterwards.
    void sort_by(const uint64_t* d_word, uint64_t n, unsigned long long* d_acc, hipStream_t s) {
        if (!n) return;
        unsigned long long oa[2] = {0ull, ~0ull};
        SBX_HIP(hipMemcpyAsync(d_acc + kMdAccOr, oa, sizeof oa, hipMemcpyHostToDevice, s));
        launch_md_gather_keys(d_word, val[at].p, n, key[at].p, d_acc, s);
        SBX_HIP(hipMemcpyAsync(oa, d_acc + kMdAccOr, sizeof oa, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        uint32_t shifts[8], bits = 0;
        const uint32_t n_passes = sortc::plan_passes(oa[0] ^ oa[1], shifts, &bits);
        for (uint32_t p = 0; p < n_passes; ++p, at ^= 1)
            launch_radix_pass(key[at].p, val[at].p, key[at ^ 1].p, val[at ^ 1].p, n, shifts[p], hist.p, hist_base.p, s);
        passes += n_passes;
    }
};

// the record numbers of [0, n) that satisfy `pred`, ascending, into d_out; returns how many
uint64_t compact(MdPred pred, const uint8_t* d_c, const uint32_t* d_mate, uint64_t n, DevBuf<uint32_t>& d_cnt, DevBuf<uint64_t>& d_base, uint32_t* d_out,
                 hipStream_t s) {
    if (!n) return 0;
    launch_md_compact(pred, d_c, d_mate, n, d_cnt.p, d_base.p, d_out, s);
    uint64_t total = 0;
    SBX_HIP(hipMemcpyAsync(&total, d_base.p + md_groups(n), 8, hipMemcpyDeviceToHost, s));
    SBX_HIP(hipStreamSynchronize(s));
    return total;
}

}  // namespace

extern "C" {

int sbx_markdup_header_text(const char* text, size_t n, const char* pg_command_line, char* out, size_t cap, size_t* out_len) {
    if (!text && n) return SBX_EINVAL;
    std::string t;
    if (!mdc::markdup_header_text(text ? text : "", n, pg_command_line, &t, nullptr)) return SBX_EFORMAT;
    return copy_to_caller(t, out, cap, out_len);
}

int sbx_markdup(const char* in_path, const char* out_path, int remove_duplicates, int level, const char* pg_command_line, int device,
                sbx_markdup_stats* stats, char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        refuse_overwrite(in_path, out_path);
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, nullptr, false);
        OutputGuard out_file(out_path);
        const int32_t n_ref = (int32_t)c->hdr.refs.size();
        std::string text, why;
        if (!mdc::markdup_header_text(c->hdr.text.data(), c->hdr.text.size(), pg_command_line, &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        const std::vector<uint8_t> header = bam_header_bytes(text, c->hdr.refs);
        const uint64_t hlen = header.size();

        // read groups -> libraries
        sortc::ParsedHeader ph;
        sortc::parse_header(c->hdr.text.data(), c->hdr.text.size(), &ph, nullptr);
        std::vector<int32_t> library_of;
        const int32_t n_lib = mdc::read_group_libraries(ph, &library_of);
        if (!mdc::key_fits(n_lib, n_ref))
            throw Error(SBX_EUNSUPPORTED, std::to_string(n_lib) + " libraries and " + std::to_string(n_ref) + " references do not fit the 64-bit position key");
        const uint32_t ref_bits = mdc::ref_bits_of(n_ref);
        std::string rg_ids;
        std::vector<uint32_t> rg_off;
        for (const sortc::HeaderLine& l : ph.rg) { rg_off.push_back((uint32_t)rg_ids.size()); rg_ids += l.id; rg_ids.push_back('\0'); }
        uint64_t hash_mask = ~0ull;
        if (const char* e = getenv("SBX_MARKDUP_HASH_BITS")) {
            const unsigned long b = strtoul(e, nullptr, 10);
            if (b < 64) hash_mask = (1ull << b) - 1ull;
        }

        const StorePlan plan = plan_record_store(c.get(), hlen, 96, "marking the duplicates of");
        const uint64_t u_first = plan.u_first;
        hipStream_t s = c->stream.get();
        DevBuf<uint8_t> d_store((size_t)plan.store_bytes + 64);
        DevBuf<char> d_rg_ids(rg_ids.size() + 1);
        DevBuf<uint32_t> d_rg_off(rg_off.size() + 1);
        DevBuf<int32_t> d_rg_lib(library_of.size() + 1);
        if (!rg_off.empty()) {
            SBX_HIP(hipMemcpyAsync(d_rg_ids.p, rg_ids.data(), rg_ids.size(), hipMemcpyHostToDevice, s));
            SBX_HIP(hipMemcpyAsync(d_rg_off.p, rg_off.data(), rg_off.size() * 4, hipMemcpyHostToDevice, s));
            SBX_HIP(hipMemcpyAsync(d_rg_lib.p, library_of.data(), library_of.size() * 4, hipMemcpyHostToDevice, s));
        }
        DevBuf<uint64_t> d_off, d_pos_key, d_hash;
        DevBuf<uint32_t> d_len, d_score, d_rg_at;
        DevBuf<uint8_t> d_cls;
        DevBuf<unsigned long long> d_acc(kMdAccWords);
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, kMdAccWords * sizeof(unsigned long long), s));
        SBX_HIP(hipStreamSynchronize(s));
        const double w1 = wall_now();

        // ---- the read pass ----
        sbx_markdup_stats st{};
        EventTimer t_k;
        uint64_t n = 0, cur = u_first;
        uint32_t n_batches = 0;
        bool too_many = false;
        unsigned long long acc[kMdAccWords] = {0};
        for_each_record_batch(c.get(), plan.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            if (n + nrec > 0xFFFFFFF0ull) { too_many = true; return false; }
            const size_t want = (size_t)(n + nrec + 2);
            grow_keeping(d_off, (size_t)n, want, s);
            grow_keeping(d_pos_key, (size_t)n, want, s);
            grow_keeping(d_hash, (size_t)n, want, s);
            grow_keeping(d_len, (size_t)n, want, s);
            grow_keeping(d_score, (size_t)n, want, s);
            grow_keeping(d_rg_at, (size_t)n, want, s);
            grow_keeping(d_cls, (size_t)n, want, s);
            t_k.start(s);
            copy_batch_to_store(c.get(), d_store.p, u_first, cur, base, next, s);
            MdEndsArgs a{};
            a.U = c->U(); a.desc = c->d_desc.p; a.n = nrec; a.u_end = next - base;
            a.n_ref = n_ref; a.ref_bits = ref_bits; a.hash_mask = hash_mask;
            a.store_delta = (int64_t)base - (int64_t)u_first;
            a.out_base = n;
            a.lib = LibTable{d_rg_ids.p, d_rg_off.p, d_rg_lib.p, (int32_t)rg_off.size()};
            a.r = MdRecords{d_off.p, d_len.p, d_cls.p, d_pos_key.p, d_score.p, d_hash.p, d_rg_at.p};
            a.acc = d_acc.p;
            launch_md_ends(a, s);
            t_k.stop(s);
            // (the next batch's K1 / K2 overwrite U and the descriptors: K10a and the copy end first)
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index; st.ms_ends += t_k.ms();
            n += nrec;
            cur = next;
            return acc[kMdAccBad] == 0;
        });
        if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
        if (acc[kMdAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kMdAccBad]));
        const uint64_t u_total = plan.u_total;
        c.reset();                                       // the batch buffers make room for the sorts and the output pieces
        const double w2 = wall_now();

        // ---- K10b: pairing ----
        Stream stream;
        stream.create();
        s = stream.get();
        const MdRecords r{d_off.p, d_len.p, d_cls.p, d_pos_key.p, d_score.p, d_hash.p, d_rg_at.p};
        DevBuf<uint32_t> d_mate((size_t)n + 2), d_cnt(md_groups(n) + 4);
        DevBuf<uint64_t> d_base(md_groups(n) + 4);
        DevBuf<uint8_t> d_dup((size_t)n + 2), d_keep((size_t)n + 2);
        WordSorter sorter;
        sorter.reserve(n);
        EventTimer t_pair, t_groups;
        t_pair.start(s);
        launch_fill32(d_mate.p, kMdNone, n, s);
        SBX_HIP(hipMemsetAsync(d_dup.p, 0, (size_t)n + 2, s));
        const uint64_t n_pairable = compact(kMdPredPairable, d_cls.p, d_mate.p, n, d_cnt, d_base, sorter.idx(), s);
        sorter.sort_by(d_hash.p, n_pairable, d_acc.p, s);
        launch_md_pair_runs(sorter.keys(), sorter.idx(), n_pairable, d_store.p, r, d_mate.p, s);
        t_pair.stop(s);
        SBX_HIP(hipStreamSynchronize(s));
        st.ms_pairing = t_pair.ms();
        d_hash.release();

        // ---- K10c: pair groups, fragment groups; K10d ----
        t_groups.start(s);
        DevBuf<uint32_t> d_first((size_t)n_pairable / 2 + 2);
        const uint64_t n_pairs = compact(kMdPredPairFirst, d_cls.p, d_mate.p, n, d_cnt, d_base, d_first.p, s);
        DevBuf<uint64_t> d_w0((size_t)n_pairs + 2), d_w1((size_t)n_pairs + 2), d_w2((size_t)n_pairs + 2), d_end2((size_t)n_pairs + 2);
        launch_md_pair_keys(d_first.p, d_mate.p, n_pairs, r, ref_bits, d_w0.p, d_w1.p, d_w2.p, d_end2.p, s);
        launch_iota(sorter.idx(), n_pairs, s);
        sorter.sort_by(d_w2.p, n_pairs, d_acc.p, s);
        sorter.sort_by(d_w1.p, n_pairs, d_acc.p, s);
        sorter.sort_by(d_w0.p, n_pairs, d_acc.p, s);
        launch_md_pair_dups(sorter.idx(), d_w0.p, d_w1.p, n_pairs, d_first.p, d_mate.p, d_dup.p, s);
        d_w1.release(); d_w2.release();
        uint64_t n_single = 0;
        {
            DevBuf<uint32_t> d_single((size_t)(n - 2 * n_pairs) + 2);
            n_single = compact(kMdPredSingle, d_cls.p, d_mate.p, n, d_cnt, d_base, d_single.p, s);
            const uint64_t m = 2 * n_pairs + n_single;
            DevBuf<uint64_t> d_v0((size_t)m + 2), d_v1((size_t)m + 2);
            DevBuf<uint32_t> d_rec((size_t)m + 2);
            launch_md_single_entries(d_w0.p, d_end2.p, n_pairs, d_single.p, n_single, r, d_v0.p, d_v1.p, d_rec.p, d_acc.p, s);
            launch_iota(sorter.idx(), m, s);
            sorter.sort_by(d_v1.p, m, d_acc.p, s);
            sorter.sort_by(d_v0.p, m, d_acc.p, s);
            launch_md_single_dups(sorter.idx(), d_v0.p, d_v1.p, d_rec.p, m, d_dup.p, s);
            SBX_HIP(hipStreamSynchronize(s));
        }
        launch_md_patch_flags(d_store.p, d_off.p, d_dup.p, n, remove_duplicates ? 1u : 0u, d_keep.p, d_acc.p, s);
        // the records that are written, in file order
        DevBuf<uint32_t> d_perm((size_t)n + 2);
        uint64_t n_out = n;
        if (remove_duplicates) n_out = compact(kMdPredKeep, d_keep.p, nullptr, n, d_cnt, d_base, d_perm.p, s);
        else launch_iota(d_perm.p, n, s);
        t_groups.stop(s);
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        st.ms_groups = t_groups.ms();
        const uint32_t n_passes = sorter.passes;
        sorter = WordSorter();
        d_w0.release(); d_end2.release(); d_first.release(); d_mate.release(); d_dup.release(); d_keep.release();
        d_pos_key.release(); d_score.release(); d_rg_at.release(); d_cls.release();

        // ---- the output ----
        DevBuf<uint64_t> d_out_off((size_t)n_out + 2);
        const WrittenBam w = write_store_output(out_file, header, d_store.p, d_off.p, d_len, d_perm.p, n_out, d_out_off.p, level,
                                                remove_duplicates ? nullptr : &acc[kMdAccBytes], "records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = w.w_planned, w4 = wall_now();
        st.n_records_in = n; st.n_records_out = n_out;
        st.n_end_pairs = n_pairs; st.n_single_ends = n_single; st.n_unmatched_pairs = acc[kMdAccUnmatched]; st.n_duplicates = acc[kMdAccDup];
        st.inflated_bytes = u_total; st.stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.n_sort_passes = n_passes; st.n_batches = n_batches;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (w4 - w0) * 1e3;
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] markdup: n_records_in=%llu n_records_out=%llu n_end_pairs=%llu n_single_ends=%llu n_unmatched_pairs=%llu "
                            "n_duplicates=%llu inflated_bytes=%llu stream_bytes=%llu compressed_bytes=%llu n_sort_passes=%u n_batches=%u "
                            "ms_inflate=%.2f ms_index=%.2f ms_ends=%.2f ms_pairing=%.2f ms_groups=%.2f ms_gather=%.2f ms_deflate=%.2f "
                            "ms_total_wall=%.1f (open %.1f, read pass %.1f, duplicates %.1f, write %.1f)\n",
                    (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_out, (unsigned long long)st.n_end_pairs,
                    (unsigned long long)st.n_single_ends, (unsigned long long)st.n_unmatched_pairs, (unsigned long long)st.n_duplicates,
                    (unsigned long long)st.inflated_bytes, (unsigned long long)st.stream_bytes, (unsigned long long)st.compressed_bytes,
                    st.n_sort_passes, st.n_batches, st.ms_inflate, st.ms_index, st.ms_ends, st.ms_pairing, st.ms_groups, st.ms_gather, st.ms_deflate,
                    st.ms_total_wall, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
        if (stats) *stats = st;
    });
}

}  // extern "C"
