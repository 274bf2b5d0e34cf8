// engine_view.cpp -- sbx_view_count / sbx_view_bam: the record selection of `sambamba view` (sambamba/view.d) on the device.
//
// One index-mode pass over the input (for_each_record_batch: K1 + K2 per batch, K2 leaving the verdict of -F in RecDesc::pad); per
// batch K12a (view.hip) decides, for every record, how many times it is selected.  -c adds that up and stores nothing, so it streams
// like sbx_flagstat.  BAM output keeps the file's records in the resident store of sbx_sort_bam (engine_store.hpp); K12b writes store
// offset and length of every selected record and, for listed regions, one (region index, record ordinal) entry per overlapped
// region; the entries are ordered by region index with the stable radix sort of sort (sort_resident: file order inside a region)
// and the result -- record ordinals, possibly the same one several times -- is the permutation plan_output / write_permuted_bam
// read.  Those index d_len / d_off through the permutation and nowhere assume that it is a bijection.
//
// The whole file is read whatever the regions say: restricting the read pass through the BAI work list is not built.
#include "engine_store.hpp"
#include "markdup_core.hpp"
#include "view.hpp"
#include "view_core.hpp"

namespace {

constexpr uint32_t kNoRegion = 0xFFFFFFFEu;      // sbx_region::ref_id no record has: the selection of a BED file that names no reference of the BAM

struct ViewRegions {
    std::vector<sbx_region> list;
    bool merged = false;
    uint32_t given() const { return list.size() == 1 && list[0].ref_id == kNoRegion ? 0u : (uint32_t)list.size(); }
};

// region strings as view.d:339-358 reads them, or the BED file as parseBed leaves it
ViewRegions resolve_regions(const sbx_ctx* c, const char* const* regions, size_t n_regions, const char* bed_path) {
    ViewRegions out;
    const bool have_bed = bed_path && *bed_path;
    if (have_bed && n_regions) throw Error(SBX_EINVAL, "specifying both region and BED filename is disallowed");      // view.d:313-315
    if (n_regions && !regions) throw Error(SBX_EINVAL, "null argument");
    if (n_regions > SBX_VIEW_MAX_REGIONS)
        throw Error(SBX_EINVAL, "too many regions (" + std::to_string(n_regions) + "): at most " + std::to_string(SBX_VIEW_MAX_REGIONS) +
                                    " may be listed; use -L with a BED file");
    if (have_bed) {
        std::vector<BedInterval> ivs;
        std::vector<std::string> lines;
        if (!read_bed_file(bed_path, &ivs, &lines)) throw Error(SBX_EIO, std::string("cannot read the BED file ") + bed_path);
        out.list = bed_merged(ivs, c->hdr);
        out.merged = true;
        if (out.list.empty()) out.list.push_back({kNoRegion, 0, 0});
        return out;
    }
    for (size_t k = 0; k < n_regions; ++k) {
        if (!regions[k]) throw Error(SBX_EINVAL, "null argument");
        const std::string arg = regions[k];
        if (arg == "*") { out.list.push_back({viewc::kUnmappedRegion, 0, 0}); continue; }
        const RegionString rs = parse_region_string(arg);
        const int id = c->hdr.find_ref(rs.reference);
        if (id < 0) throw Error(SBX_EINVAL, "Reference with name " + rs.reference + " does not exist");              // reader.d:426
        sbx_region g{(uint32_t)id, rs.beg, rs.end};
        if (g.end == 0xFFFFFFFFu) g.end = (uint32_t)c->hdr.refs[(size_t)id].length;
        if (!(g.start < g.end)) throw Error(SBX_EINVAL, "region " + arg + " is empty");                              // randomaccessmanager.d:256
        out.list.push_back(g);
    }
    return out;
}

void check_opts(const sbx_filter* filter, const sbx_view_opts* opts, uint64_t* threshold) {
    check_filter(filter);
    *threshold = 0;
    if (opts && opts->subsample && !viewc::subsample_threshold(opts->fraction, threshold))
        throw Error(SBX_EINVAL, "the subsampling fraction must be a number that is not negative");
}

ViewSelectArgs select_args(sbx_ctx* c, const sbx_view_opts* opts, uint64_t threshold, const ViewRegions& regions, const sbx_region* d_regions,
                           uint64_t nrec, uint64_t u_end, unsigned long long* d_acc) {
    ViewSelectArgs a{};
    a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = u_end;
    if (opts) {
        a.flags_set = opts->flags_set; a.flags_unset = opts->flags_unset;
        a.subsample = opts->subsample ? 1u : 0u; a.seed = opts->seed; a.threshold = threshold;
    }
    a.regions = d_regions; a.n_regions = (uint32_t)regions.list.size(); a.regions_merged = regions.merged ? 1u : 0u;
    a.acc = d_acc;
    return a;
}

void upload_regions(const ViewRegions& regions, DevBuf<sbx_region>* d, hipStream_t s) {
    d->ensure(regions.list.size() + 1);
    if (!regions.list.empty()) SBX_HIP(hipMemcpyAsync(d->p, regions.list.data(), regions.list.size() * sizeof(sbx_region), hipMemcpyHostToDevice, s));
}

void print_timing(const sbx_view_stats& st, const char* sink) {
    if (!getenv("SBX_TIMING")) return;
    fprintf(stderr, "[sbx] view: sink=%s n_records_in=%llu n_records_selected=%llu n_entries_out=%llu inflated_bytes=%llu stream_bytes=%llu "
                    "compressed_bytes=%llu n_regions=%u n_sort_passes=%u n_batches=%u ms_inflate=%.2f ms_index=%.2f ms_select=%.3f ms_emit=%.3f "
                    "ms_sort=%.2f ms_gather=%.2f ms_deflate=%.2f ms_total_wall=%.1f\n",
            sink, (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_selected, (unsigned long long)st.n_entries_out,
            (unsigned long long)st.inflated_bytes, (unsigned long long)st.stream_bytes, (unsigned long long)st.compressed_bytes, st.n_regions,
            st.n_sort_passes, st.n_batches, st.ms_inflate, st.ms_index, st.ms_select, st.ms_emit, st.ms_sort, st.ms_gather, st.ms_deflate,
            st.ms_total_wall);
}

}  // namespace

extern "C" {

int sbx_view_num_filter(const char* text, uint16_t* flags_set, uint16_t* flags_unset) {
    if (!flags_set || !flags_unset) return SBX_EINVAL;
    return viewc::parse_num_filter(text, flags_set, flags_unset) ? SBX_OK : SBX_EINVAL;
}

int sbx_view_reference_info(sbx_ctx* c, char* out, size_t cap, size_t* out_len) {
    if (!c) return SBX_EINVAL;
    std::vector<std::string> names;
    std::vector<int64_t> lengths;
    for (const RefSeq& r : c->hdr.refs) { names.push_back(r.name); lengths.push_back(r.length); }
    return copy_to_caller(viewc::reference_info_json(names, lengths), out, cap, out_len);
}

int sbx_view_count(const char* in_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions, size_t n_regions,
                   const char* bed_path, int device, uint64_t* count, sbx_view_stats* stats, char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!in_path || !count) throw Error(SBX_EINVAL, "null argument");
        uint64_t threshold = 0;
        check_opts(filter, opts, &threshold);
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, filter, true);
        const ViewRegions sel = resolve_regions(c.get(), regions, n_regions, bed_path);
        hipStream_t s = c->stream.get();
        DevBuf<sbx_region> d_regions;
        upload_regions(sel, &d_regions, s);
        DevBuf<unsigned long long> d_acc(kViewAccWords);
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, kViewAccWords * sizeof(unsigned long long), s));
        sbx_view_stats st{};
        EventTimer t_k;
        uint64_t n_in = 0;
        uint32_t n_batches = 0;
        for_each_record_batch(c.get(), index_batch_bytes(), &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            t_k.start(s);
            launch_view_select(select_args(c.get(), opts, threshold, sel, d_regions.p, nrec, next - base, d_acc.p), s);
            t_k.stop(s);
            // (the next batch's K2 overwrites these descriptors, and may reallocate them, from the host side: K12a ends first)
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index;
            if (nrec) st.ms_select += t_k.ms();
            n_in += nrec;
            return true;
        });
        unsigned long long acc[kViewAccWords] = {0};
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        if (acc[kViewAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kViewAccBad]));
        st.n_records_in = n_in; st.n_records_selected = acc[kViewAccRecords]; st.n_entries_out = acc[kViewAccEntries];
        st.inflated_bytes = c->blocks.out_off.back();
        st.n_regions = sel.given(); st.n_batches = n_batches;
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        print_timing(st, "count");
        *count = acc[kViewAccEntries];
        if (stats) *stats = st;
    });
}

int sbx_view_bam(const char* in_path, const char* out_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions,
                 size_t n_regions, const char* bed_path, const char* pg_command_line, int level, int with_index, int device,
                 sbx_view_stats* stats, char* err, size_t errlen) {
    const bool to_stdout = !out_path || !strcmp(out_path, "-");
    const char* const path = to_stdout ? "/dev/stdout" : out_path;
    const int rc = run_entry(err, errlen, [&] {
        if (!in_path) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        if (to_stdout && with_index) throw Error(SBX_EINVAL, "an output on stdout cannot be indexed");
        if (!to_stdout) refuse_overwrite(in_path, path);
        uint64_t threshold = 0;
        check_opts(filter, opts, &threshold);
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, filter, true);
        OutputGuard out_file(path, to_stdout);
        const ViewRegions sel = resolve_regions(c.get(), regions, n_regions, bed_path);
        const bool listed = !sel.merged && !sel.list.empty();
        std::string text, why;
        if (!mdc::markdup_header_text(c->hdr.text.data(), c->hdr.text.size(), pg_command_line, &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        const std::vector<uint8_t> header = bam_header_bytes(text, c->hdr.refs);
        const uint64_t hlen = header.size();

        const StorePlan plan = plan_record_store(c.get(), hlen, 48, "selecting records of");
        const uint64_t u_first = plan.u_first;
        hipStream_t s = c->stream.get();
        DevBuf<uint8_t> d_store((size_t)plan.store_bytes + 64);
        DevBuf<sbx_region> d_regions;
        upload_regions(sel, &d_regions, s);
        DevBuf<uint64_t> d_off, d_entry_key, d_group_entry_base, d_group_record_base;
        DevBuf<uint32_t> d_len, d_entry_rec, d_count, d_group_entries, d_group_records;
        DevBuf<unsigned long long> d_acc(kViewAccWords);
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, kViewAccWords * sizeof(unsigned long long), s));
        SBX_HIP(hipStreamSynchronize(s));

        // ---- the read pass ----
        sbx_view_stats st{};
        EventTimer t_a, t_b;
        uint64_t n_in = 0, n_rec = 0, n_ent = 0, cur = u_first;
        uint32_t n_batches = 0;
        bool too_many = false;
        unsigned long long acc[kViewAccWords] = {0};
        for_each_record_batch(c.get(), plan.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            const uint32_t groups = view_groups(nrec);
            d_count.ensure((size_t)nrec + 2);
            d_group_entries.ensure(groups + 4); d_group_records.ensure(groups + 4);
            d_group_entry_base.ensure(groups + 4); d_group_record_base.ensure(groups + 4);
            t_a.start(s);
            copy_batch_to_store(c.get(), d_store.p, u_first, cur, base, next, s);
            ViewSelectArgs a = select_args(c.get(), opts, threshold, sel, d_regions.p, nrec, next - base, d_acc.p);
            a.with_lengths = 1;
            a.count = d_count.p; a.group_entries = d_group_entries.p; a.group_records = d_group_records.p;
            launch_view_select(a, s);
            if (nrec) {
                launch_count_scan(d_group_entries.p, groups, d_group_entry_base.p, nullptr, 0, s);
                launch_count_scan(d_group_records.p, groups, d_group_record_base.p, nullptr, 0, s);
            }
            t_a.stop(s);
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_inflate += c->stats.ms_inflate; st.ms_index += c->stats.ms_index; st.ms_select += t_a.ms();
            n_in += nrec;
            cur = next;
            if (acc[kViewAccBad]) return false;
            if (acc[kViewAccEntries] > 0xFFFFFFF0ull) { too_many = true; return false; }
            // the arrays grow to what the batch selected, then K12b fills them
            grow_keeping(d_off, (size_t)n_rec, (size_t)acc[kViewAccRecords] + 2, s);
            grow_keeping(d_len, (size_t)n_rec, (size_t)acc[kViewAccRecords] + 2, s);
            if (listed) {
                grow_keeping(d_entry_key, (size_t)n_ent, (size_t)acc[kViewAccEntries] + 2, s);
                grow_keeping(d_entry_rec, (size_t)n_ent, (size_t)acc[kViewAccEntries] + 2, s);
            }
            ViewEmitArgs b{};
            b.s = a;
            b.group_entry_base = d_group_entry_base.p; b.group_record_base = d_group_record_base.p;
            b.store_delta = (int64_t)base - (int64_t)u_first;
            b.record_base = n_rec; b.entry_base = n_ent;
            b.off = d_off.p; b.len = d_len.p;
            b.entry_key = listed ? d_entry_key.p : nullptr; b.entry_rec = listed ? d_entry_rec.p : nullptr;
            t_b.start(s);
            launch_view_emit(b, s);
            t_b.stop(s);
            // (the next batch's K1 / K2 overwrite U and the descriptors: K12b and the copy end first)
            SBX_HIP(hipStreamSynchronize(s));
            if (nrec) st.ms_emit += t_b.ms();
            n_rec = acc[kViewAccRecords];
            n_ent = acc[kViewAccEntries];
            return true;
        });
        if (acc[kViewAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kViewAccBad]));
        if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 output records");
        if (!listed && n_ent != n_rec) throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_ent) + " entries for " + std::to_string(n_rec) + " records");
        const uint64_t u_total = plan.u_total;
        c.reset();                                       // the batch buffers make room for the sort and the output pieces
        d_count.release(); d_group_entries.release(); d_group_records.release(); d_group_entry_base.release(); d_group_record_base.release();

        // ---- the order of the entries ----
        Stream stream;
        stream.create();
        s = stream.get();
        const uint64_t n = n_ent;
        DevBuf<uint32_t> d_perm((size_t)n + 2);
        ResidentOrder order;
        if (listed && sel.list.size() > 1) {
            // keys are region indices: what varies lies below the width of the largest one
            const uint64_t varying = (1ull << sortc::bit_width64((uint64_t)sel.list.size() - 1)) - 1ull;
            d_entry_key.ensure((size_t)n + 2);
            sort_resident(d_entry_key.p, n, varying, s, &order);
            EventTimer t_c;
            t_c.start(s);
            launch_view_compose(d_entry_rec.p, order.perm, n, d_perm.p, s);
            t_c.stop(s);
            SBX_HIP(hipStreamSynchronize(s));
            st.ms_sort = order.ms_sort + (n ? t_c.ms() : 0.0);
            st.n_sort_passes = order.n_passes;
            order = ResidentOrder();
        } else if (listed) {
            if (n) SBX_HIP(hipMemcpyAsync(d_perm.p, d_entry_rec.p, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
        } else {
            launch_iota(d_perm.p, n, s);
        }
        d_entry_key.release(); d_entry_rec.release();
        d_len.ensure(2);                                 // (nothing selected: the arrays were never grown)
        d_off.ensure(2);
        DevBuf<uint64_t> d_out_off((size_t)n + 2);
        const WrittenBam w = write_store_output(out_file, header, d_store.p, d_off.p, d_len, d_perm.p, n, d_out_off.p, level,
                                                &acc[kViewAccBytes], "selected records", s, &st.ms_gather);
        out_file.disarm();
        st.n_records_in = n_in; st.n_records_selected = n_rec; st.n_entries_out = n;
        st.inflated_bytes = u_total; st.stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.n_regions = sel.given(); st.n_batches = n_batches;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        print_timing(st, "bam");
        if (stats) *stats = st;
    });
    // (the index is a pass of its own and not part of the figures)
    return rc != SBX_OK ? rc : index_written_bam(path, with_index, device, err, errlen);
}

}  // extern "C"
