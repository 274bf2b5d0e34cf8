// engine_view.cpp -- sbx_view_run, and sbx_view_count / sbx_view_bam / sbx_view_sam as that call with valid_only = 0: the record
// selection of `sambamba view` (sambamba/view.d) on the device.  With valid_only (`view -v`) K19 (valid.hip) runs on every batch in
// front of K12a, which then selects no record whose mask is not 0; its time is part of ms_select.
//
// One index-mode pass over the input (for_each_record_batch: K1 + K2 per batch, K2 leaving the verdict of -F in RecDesc::pad); per
// batch K12a (view.hip) decides, for every record, how many times it is selected.  -c adds that up and stores nothing, so it streams
// like sbx_flagstat.  BAM output keeps the file's records in the resident store of sbx_sort_bam (engine_store.hpp); K12b writes store
// offset and length of every selected record and, for listed regions, one (region index, record ordinal) entry per overlapped
// region; the entries are ordered by region index with the stable radix sort of sort (sort_resident: file order inside a region)
// and the result -- record ordinals, possibly the same one several times -- is the permutation plan_output / write_permuted_bam
// read.  Those index d_len / d_off through the permutation and nowhere assume that it is a bijection.
//
// sbx_view_sam is a third sink over the same store and permutation: K13a (sam.hip) measures the line of every entry, a scan gives the
// 64-bit offsets, and K13b writes the text piece by piece -- two device and two pinned buffers, so that the copy and the write of
// a piece overlap the kernel of the next.
//
// An output in file order -- no region, one listed region, -L -- whose records do not fit the store (or SBX_STREAM_WINDOW_BYTES) keeps
// none (ViewJob::plan_store decides).  view_bam_streamed hands every batch, while it is in U, to the StreamedOutput of
// engine_streamout.hpp (K21, stream.hip); view_sam_streamed runs K12b, K13a and K13b per batch with the batch as the store.
//
// The shape of the file: ViewJob is the prologue and the epilogue of every sink -- what it derives from the validated
// sbx_view_request (threshold, context, regions, the indexed read, header text, the output path), the wall time and the timing line.
// SelectStep is the one per-batch selection step (K19, K12a, the group scans, the read-back, the checks); the count sink, the
// resident store (select_resident) and both streamed sinks call it and say what K12a is to leave behind.  view_count, view_bam and
// view_sam take the request itself.
//
// sbx_view_run and the three calls of before it read the whole file whatever the regions say (their stats promise n_records_in =
// the records of the file, and they need no .bai).  sbx_view_run_indexed reads only the blocks the .bai names for the regions: the
// runs of build_runs over all regions of the call, the stretch of `*` (index_starts.hpp), joined and cut into batches by the planner
// of view_index_core.hpp.  Both paths feed the same consumers (read_batches); K12a / K12b select over whatever was described, so the
// result is the one of the whole-file pass as long as the file is in coordinate order -- which K12c checks on every batch that was
// read (SBX_ENOTSORTED).  The record store of the BAM and SAM sinks is then sized by the inflated bytes of the runs' blocks.
#include "engine_streamout.hpp"
#include "index_starts.hpp"
#include "markdup_core.hpp"
#include "sam.hpp"
#include "valid.hpp"
#include "view.hpp"
#include "view_core.hpp"
#include "view_index_core.hpp"

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

// view -v: K19 in front of K12a.  run() leaves the masks of the batch's records and returns them; null when the option is off.
struct ValidPass {
    bool on = false;
    DevBuf<uint16_t> mask;
    DevBuf<unsigned long long> acc;
    uint64_t rec_base = 0;
    void init(bool valid_only, hipStream_t s) {
        on = valid_only;
        if (!on) return;
        unsigned long long zero[kValidAccWords] = {0};
        zero[kValidAccFirst] = kValidNone;
        acc.alloc(kValidAccWords);
        SBX_HIP(hipMemcpyAsync(acc.p, zero, sizeof zero, hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));
    }
    const uint16_t* run(sbx_ctx* c, uint64_t nrec, uint64_t u_end, hipStream_t s) {
        if (!on) return nullptr;
        mask.ensure((size_t)nrec + 2);
        launch_valid_masks(ValidArgs{c->U(), c->d_desc.p, nrec, u_end, rec_base, mask.p, acc.p}, s);
        rec_base += nrec;
        return mask.p;
    }
};

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

// ---- the read pass: the whole file, or the runs the index names for the regions ----
void print_index_timing(const sbx_view_index_stats& ix) {
    if (!getenv("SBX_TIMING")) return;
    fprintf(stderr, "[sbx] view-index: blocks_in_file=%llu blocks_read=%llu runs=%llu compressed_bytes_read=%llu inflated_bytes_read=%llu ms_plan=%.3f\n",
            (unsigned long long)ix.blocks_in_file, (unsigned long long)ix.blocks_read, (unsigned long long)ix.runs,
            (unsigned long long)ix.compressed_bytes_read, (unsigned long long)ix.inflated_bytes_read, ix.ms_plan);
}

struct IndexedRead {
    bool on = false;                // false: the whole-file pass
    std::vector<FileRun> runs;      // joined, ascending
    uint64_t store_bytes = 0;       // inflated bytes of their blocks: what the record store has to hold at most
};

// From the regions to the run list.  index_mode OFF, no region and no BED file, or AUTO without a .bai: the whole-file pass.
IndexedRead plan_indexed_read(const sbx_ctx* c, const char* in_path, const ViewRegions& sel, int index_mode, sbx_view_index_stats* ix_out) {
    const double w0 = wall_now();
    const BlockTable& bt = c->blocks;
    const uint32_t nbk = (uint32_t)bt.size();
    IndexedRead rd;
    sbx_view_index_stats ix{};
    ix.blocks_in_file = nbk;
    if (index_mode != SBX_VIEW_INDEX_OFF && index_mode != SBX_VIEW_INDEX_REQUIRED && index_mode != SBX_VIEW_INDEX_AUTO)
        throw Error(SBX_EINVAL, "unknown index mode " + std::to_string(index_mode));
    if (index_mode != SBX_VIEW_INDEX_OFF && !sel.list.empty()) {
        if (c->has_index) rd.on = true;
        else if (index_mode == SBX_VIEW_INDEX_REQUIRED) throw Error(SBX_ENOINDEX, std::string("the input has no index: ") + in_path + ".bai is needed");
    }
    if (!rd.on) {
        ix.blocks_read = nbk; ix.runs = nbk ? 1 : 0; ix.compressed_bytes_read = c->file.size; ix.inflated_bytes_read = bt.out_off.back();
        ix.ms_plan = (wall_now() - w0) * 1e3;
        if (index_mode != SBX_VIEW_INDEX_OFF) print_index_timing(ix);
        if (ix_out) *ix_out = ix;
        return rd;
    }
    if (c->bai.refs.size() != c->hdr.refs.size())
        throw Error(SBX_EFORMAT, "the index names " + std::to_string(c->bai.refs.size()) + " references, the header of the BAM " +
                                     std::to_string(c->hdr.refs.size()) + ": the .bai does not belong to this file");
    std::vector<sbx_region> placed;
    bool star = false;
    for (const sbx_region& g : sel.list) {
        if (g.ref_id == viewc::kUnmappedRegion) star = true;
        else if (g.ref_id != kNoRegion) placed.push_back(g);
    }
    if (!placed.empty()) rd.runs = build_runs(c, placed, true);
    if (star) viewidx::unmapped_tail(bt.out_off.data(), nbk, unmapped_start(c, index_starts(c)), &rd.runs);
    rd.runs = join_runs(std::move(rd.runs), 1);
    viewidx::runs_cost(rd.runs, bt.out_off.data(), &ix.blocks_read, &rd.store_bytes);
    ix.runs = rd.runs.size();
    ix.inflated_bytes_read = rd.store_bytes;
    for (const FileRun& r : rd.runs) ix.compressed_bytes_read += bt.comp_off[r.blk1 - 1] + bt.comp_len[r.blk1 - 1] + 8 - bt.coffset[r.blk0];
    ix.ms_plan = (wall_now() - w0) * 1e3;
    print_index_timing(ix);
    if (ix_out) *ix_out = ix;
    return rd;
}

// One batch of the read pass as its consumer sees it: records [0, nrec) of c->d_desc / c->d_rec_ref, their rec_off offsets of U.
struct ViewBatch {
    uint64_t nrec;
    uint64_t u_end;                 // no record of the batch ends behind this offset of U
    uint64_t keep_lo, keep_hi;      // the bytes of U from the batch's first record to behind its last: what a record store keeps
};

// K12c over the batch that was just described; the key of its last record is carried to the next one
struct OrderCheck {
    DevBuf<uint32_t> unsorted;
    DevBuf<unsigned long long> last;
    uint64_t prev_key = 0;
    void run(sbx_ctx* c, uint64_t nrec, hipStream_t s) {
        if (!nrec) return;
        unsorted.ensure(1); last.ensure(1);
        uint32_t flag = 0;
        unsigned long long key = 0;
        SBX_HIP(hipMemsetAsync(unsorted.p, 0, 4, s));
        launch_view_order(c->d_desc.p, c->d_rec_ref.p, nrec, prev_key, unsorted.p, last.p, s);
        SBX_HIP(hipMemcpyAsync(&flag, unsorted.p, 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(&key, last.p, 8, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        if (flag) throw Error(SBX_ENOTSORTED, "the records the index names for the regions are not in coordinate order: the .bai does not describe this file");
        prev_key = key;
    }
};

// consume(ViewBatch) once per batch, in file order; it returns false to stop the pass.  *inflated receives the bytes K1 wrote.
template <class Consume>
void read_batches(sbx_ctx* c, const IndexedRead& rd, uint64_t batch_u, uint32_t* n_batches, uint64_t* inflated, Consume&& consume) {
    const BlockTable& bt = c->blocks;
    *n_batches = 0;
    if (!rd.on) {
        uint64_t cur = c->hdr.first_record_off;
        for_each_record_batch(c, batch_u, n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            const ViewBatch b{nrec, next - base, cur - base, next - base};
            cur = next;
            return consume(b);
        });
        *inflated = bt.out_off.back();
        return;
    }
    *inflated = 0;
    viewidx::Planner planner(rd.runs, bt.out_off.data(), batch_u);
    std::vector<FileRun> batch;
    OrderCheck order;
    while (planner.next(&batch)) {
        run_impl(c, {}, false, &batch);
        const WorkList& wl = c->wl;
        *inflated += wl.u_bytes;
        // an open-ended piece stops in front of the record that straddles its last block boundary (describe_record_run)
        const bool stopped = batch.size() == 1 && batch[0].open_end && c->index_straddler != kOffUnknown;
        const uint64_t keep_hi = stopped ? c->index_straddler : wl.chain.back().u_end;
        const uint64_t stop = stopped ? bt.out_off[batch[0].blk0] + c->index_straddler : batch.back().ue;
        if (!planner.advance(stop)) continue;           // not one whole record in the piece: again, longer
        ++*n_batches;
        const uint64_t nrec = c->primary_records;
        order.run(c, nrec, c->stream.get());
        if (!consume(ViewBatch{nrec, keep_hi, wl.chain.front().u_beg, keep_hi})) return;
    }
}

// The output order is the file order when no region orders it: no region, one listed region, or the merged list of a BED file.
bool in_file_order(const ViewRegions& sel) { return sel.merged || sel.list.size() <= 1; }

// ---- what every sink derives from the request: the prologue and the epilogue of a call ----
struct ViewJob {
    const sbx_view_request& q;
    const bool to_stdout;
    const char* const path;         // of the output; "/dev/stdout" for none or "-"
    double w0 = 0;
    uint64_t threshold = 0;         // of -s
    Standalone c;
    OutputGuard out_file;
    ViewRegions sel;
    IndexedRead rd;
    std::string text;               // header text of the output, where the sink has one

    static const char* path_of(const sbx_view_request& q) { return !q.out_path || !strcmp(q.out_path, "-") ? "/dev/stdout" : q.out_path; }
    explicit ViewJob(const sbx_view_request& request)
        : q(request), to_stdout(path_of(request) != request.out_path), path(path_of(request)), out_file(path, to_stdout) {}
    // Behind the sink's own argument checks: the options, the input, the regions, the read through the index and -- with_text -- the
    // header text.
    void open(int index_mode, bool with_text, sbx_view_index_stats* ix) {
        check_opts(q.filter, q.opts, &threshold);
        w0 = wall_now();
        c = open_record_pass(q.in_path, q.device, q.filter, true);
        sel = resolve_regions(c.get(), q.regions, q.n_regions, q.bed_path);
        rd = plan_indexed_read(c.get(), q.in_path, sel, index_mode, ix);
        std::string why;
        if (with_text && !mdc::markdup_header_text(c->hdr.text.data(), c->hdr.text.size(), q.pg_command_line, &text, &why))
            throw Error(SBX_EFORMAT, "SAM header: " + why);
    }
    // The resident store of select_resident -- it holds the records of the file, or, indexed, the bytes of the runs -- or nothing: the
    // sink streams.  In file order that is when the hook asks for it or the store does not fit; two or more listed regions need the
    // store, and its refusal is theirs.  hlen / per_record: bytes of the sink's header and of the per-record arrays it will add.
    std::optional<StorePlan> plan_store(uint64_t hlen, uint64_t per_record, uint64_t hook) const {
        auto plan = [&] {
            return rd.on ? plan_store_bytes(rd.store_bytes, hlen, per_record, "selecting records of", "the blocks the index names for the regions do")
                         : plan_record_store(c.get(), hlen, per_record, "selecting records of");
        };
        if (!in_file_order(sel)) return plan();
        if (hook) return std::nullopt;
        return plan_if_fits(plan);
    }
    // the epilogue
    void finish(sbx_view_stats& st, const char* sink, sbx_view_stats* stats) const {
        st.ms_total_wall = (wall_now() - w0) * 1e3;
        print_timing(st, sink);
        if (stats) *stats = st;
    }
};

// ---- the one selection step of all sinks ----
// Per batch: K19 with -v, K12a, the scans of the group sums, the accumulators read back; the checks on them, raised when the batch
// that trips them is met; at the end the errors and what the pass gives the stats.  What K12a leaves next to the accumulators is the
// sink's choice: the count sink wants nothing, the streamed BAM sink lengths checked and the entries of every record (K21 reads
// them), and K12b -- the resident store, the streamed SAM sink -- the group sums and their scans as well.
struct SelectWants { bool lengths, counts, groups; };
struct SelectStep {
    const ViewJob& job;
    const SelectWants wants;
    DevBuf<sbx_region> d_regions;
    DevBuf<uint32_t> d_count, d_group_entries, d_group_records;
    DevBuf<uint64_t> d_group_entry_base, d_group_record_base;
    PassBooks<kViewAccWords> books;
    ValidPass valid;
    EventTimer t_a;
    double ms_select = 0;
    unsigned long long before[kViewAccWords] = {0};    // books.acc in front of the last batch
    uint64_t inflated = 0;
    uint32_t n_batches = 0;
    bool too_many = false;
    ViewSelectArgs a{};                                 // K12a's arguments for the last batch

    SelectStep(const ViewJob& j, SelectWants w, hipStream_t s) : job(j), wants(w) {
        upload_regions(job.sel, &d_regions, s);
        books.init(s);
        valid.init(job.q.valid_only != 0, s);
    }
    // store_at: where the bytes of the batch a record store keeps go -- queued inside ms_select's interval --, or null.
    // false: a check tripped (refuse_bad() / refuse_output() say which); a sink with an output stops the pass there.
    bool run(const ViewBatch& vb, uint8_t* store_at, hipStream_t s) {
        sbx_ctx* c = job.c.get();
        const uint64_t nrec = vb.nrec, kept = vb.keep_hi - vb.keep_lo;
        const uint32_t n_groups = view_groups(nrec);
        memcpy(before, books.acc, sizeof before);
        if (wants.counts) d_count.ensure((size_t)nrec + 2);
        if (wants.groups) {
            d_group_entries.ensure(n_groups + 4); d_group_records.ensure(n_groups + 4);
            d_group_entry_base.ensure(n_groups + 4); d_group_record_base.ensure(n_groups + 4);
        }
        t_a.start(s);
        // the batch's records go behind those of the batches before
        if (store_at && kept) SBX_HIP(hipMemcpyAsync(store_at, c->U() + vb.keep_lo, kept, hipMemcpyDeviceToDevice, s));
        a = ViewSelectArgs{};
        a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = vb.u_end;
        if (const sbx_view_opts* opts = job.q.opts) {
            a.flags_set = opts->flags_set; a.flags_unset = opts->flags_unset;
            a.subsample = opts->subsample ? 1u : 0u; a.seed = opts->seed; a.threshold = job.threshold;
        }
        a.regions = d_regions.p; a.n_regions = (uint32_t)job.sel.list.size(); a.regions_merged = job.sel.merged ? 1u : 0u;
        a.acc = books.d_acc.p;
        a.invalid = valid.run(c, nrec, vb.u_end, s);
        a.with_lengths = wants.lengths ? 1u : 0u;
        a.count = wants.counts ? d_count.p : nullptr;
        if (wants.groups) { a.group_entries = d_group_entries.p; a.group_records = d_group_records.p; }
        launch_view_select(a, s);
        if (wants.groups && nrec) {
            launch_count_scan(d_group_entries.p, n_groups, d_group_entry_base.p, s);
            launch_count_scan(d_group_records.p, n_groups, d_group_record_base.p, s);
        }
        t_a.stop(s);
        // (the next batch's K1 / K2 overwrite U and the descriptors, and may reallocate them: K12a and the copy end first)
        books.read_back(c, nrec, s);
        ms_select += t_a.ms();
        too_many = too_many || books.acc[kViewAccEntries] > 0xFFFFFFF0ull;
        return !books.acc[kViewAccBad] && !too_many;
    }
    void refuse_bad() const {
        if (books.acc[kViewAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(books.acc[kViewAccBad]));
    }
    // for a sink with an output, behind refuse_bad(); one_entry_per_record: the output is in file order
    void refuse_output(bool one_entry_per_record) const {
        const unsigned long long n_ent = books.acc[kViewAccEntries], n_rec = books.acc[kViewAccRecords];
        if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 output records");
        if (one_entry_per_record && n_ent != n_rec)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_ent) + " entries for " + std::to_string(n_rec) + " records");
    }
    void fill(sbx_view_stats* st) const {
        st->n_records_in = books.n; st->n_records_selected = books.acc[kViewAccRecords]; st->n_entries_out = books.acc[kViewAccEntries];
        st->inflated_bytes = inflated;
        st->n_regions = job.sel.given(); st->n_batches = n_batches;
        st->ms_inflate = books.ms_inflate; st->ms_index = books.ms_index; st->ms_select = ms_select;
    }
};

// ---- what the BAM and the SAM sink share: the read pass and the order of the entries ----
// The records of the file in the resident store and the selected entries in output order: entry i is record perm[i], len[perm[i]]
// bytes at store + off[perm[i]].
struct SelectedRecords {
    DevBuf<uint8_t> store;
    DevBuf<uint64_t> off;
    DevBuf<uint32_t> len, perm;
    uint64_t n = 0;                 // entries
    unsigned long long record_bytes = 0;    // their record bytes, as K12a added them up
    Stream stream;                  // what follows the read pass runs on it (declared last: it is waited for before the buffers go)
};

// Reads the file (K1, K2, K12a, K12b per batch; the records go to the store `plan` describes), closes the context and orders the
// entries (K9b over the region index for listed regions).  Fills the counts and the times of the passes into *st.
void select_resident(ViewJob& job, const StorePlan& plan, SelectedRecords* out, sbx_view_stats* st_out) {
    sbx_view_stats& st = *st_out;
    const ViewRegions& sel = job.sel;
    const bool listed = !sel.merged && !sel.list.empty();
    DevBuf<uint8_t>& d_store = out->store;
    DevBuf<uint64_t>& d_off = out->off;
    DevBuf<uint32_t>& d_len = out->len;
    DevBuf<uint32_t>& d_perm = out->perm;
    Stream& stream = out->stream;
    hipStream_t s = job.c->stream.get();
    d_store = DevBuf<uint8_t>((size_t)plan.store_bytes + 64);
    SelectStep pick(job, SelectWants{true, true, true}, s);
    const unsigned long long* acc = pick.books.acc;
    DevBuf<uint64_t> d_entry_key;
    DevBuf<uint32_t> d_entry_rec;

    // ---- the read pass ----
    EventTimer t_b;
    uint64_t store_at = 0;
    read_batches(job.c.get(), job.rd, plan.batch_u, &pick.n_batches, &pick.inflated, [&](const ViewBatch& vb) -> bool {
        const uint64_t kept = vb.keep_hi - vb.keep_lo;
        if (store_at + kept > plan.store_bytes) throw Error(SBX_EFORMAT, "internal error: the batches hold more bytes than the record store was planned for");
        const bool go_on = pick.run(vb, d_store.p + store_at, s);
        const int64_t store_delta = (int64_t)store_at - (int64_t)vb.keep_lo;
        store_at += kept;
        if (!go_on) return false;
        // the arrays grow to what the batch selected, then K12b fills them
        const uint64_t n_rec = pick.before[kViewAccRecords], n_ent = pick.before[kViewAccEntries];
        grow_keeping(d_off, (size_t)n_rec, (size_t)acc[kViewAccRecords] + 2, s);
        grow_keeping(d_len, (size_t)n_rec, (size_t)acc[kViewAccRecords] + 2, s);
        if (listed) {
            grow_keeping(d_entry_key, (size_t)n_ent, (size_t)acc[kViewAccEntries] + 2, s);
            grow_keeping(d_entry_rec, (size_t)n_ent, (size_t)acc[kViewAccEntries] + 2, s);
        }
        ViewEmitArgs b{};
        b.s = pick.a;
        b.group_entry_base = pick.d_group_entry_base.p; b.group_record_base = pick.d_group_record_base.p;
        b.store_delta = store_delta;
        b.record_base = n_rec; b.entry_base = n_ent;
        b.off = d_off.p; b.len = d_len.p;
        b.entry_key = listed ? d_entry_key.p : nullptr; b.entry_rec = listed ? d_entry_rec.p : nullptr;
        t_b.start(s);
        launch_view_emit(b, s);
        t_b.stop(s);
        // (the next batch's K1 / K2 overwrite U and the descriptors: K12b ends first)
        SBX_HIP(hipStreamSynchronize(s));
        if (vb.nrec) st.ms_emit += t_b.ms();
        return true;
    });
    pick.refuse_bad();
    pick.refuse_output(!listed);
    const uint64_t n_ent = acc[kViewAccEntries];
    job.c.reset();                                   // the batch buffers make room for the sort and the output pieces
    pick.d_count.release(); pick.d_group_entries.release(); pick.d_group_records.release();
    pick.d_group_entry_base.release(); pick.d_group_record_base.release();

    // ---- the order of the entries ----
    stream.create();
    s = stream.get();
    const uint64_t n = n_ent;
    d_perm = DevBuf<uint32_t>((size_t)n + 2);
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
    out->n = n;
    out->record_bytes = acc[kViewAccBytes];
    pick.fill(&st);
}

// ---- the streamed BAM sink: no store; K12a per batch, then K21 into the staging window (engine_streamout.hpp) ----
// no more record bytes than this reach the output of a pass
uint64_t record_bytes_max(const sbx_ctx* c, const IndexedRead& rd) {
    const uint64_t u_total = c->blocks.out_off.back(), u_first = std::min<uint64_t>(c->hdr.first_record_off, u_total);
    return rd.on ? rd.store_bytes : u_total - u_first;
}
const char* iview_hint(const IndexedRead& rd) { return rd.on ? "" : "; sbx-iview reads only the blocks the index names for a region"; }

void view_bam_streamed(ViewJob& job, const std::vector<uint8_t>& header, uint64_t hook, sbx_view_stats* st, sbx_stream_stats* stream_stats) {
    sbx_ctx* c = job.c.get();
    const uint64_t stream_max = header.size() + record_bytes_max(c, job.rd);
    const StreamBudget budget(stream_max, hook, 18, "selecting records of", "18 bytes per record of it", iview_hint(job.rd));
    hipStream_t s = c->stream.get();
    StreamedOutput out(job.out_file, header, stream_max, budget, job.q.level, s);
    SelectStep pick(job, SelectWants{true, true, false}, s);
    read_batches(c, job.rd, budget.batch_u, &pick.n_batches, &pick.inflated, [&](const ViewBatch& vb) -> bool {
        if (!pick.run(vb, nullptr, s)) return false;
        PackArgs p{};
        p.U = c->U(); p.desc = c->d_desc.p; p.n = vb.nrec; p.u_end = vb.u_end;
        p.count = pick.d_count.p;
        // (the next batch's K1 / K2 overwrite U and the descriptors: add_batch returns when K21 has read them)
        out.add_batch(p, pick.books.acc[kViewAccBytes] - pick.before[kViewAccBytes]);
        return true;
    });
    pick.refuse_bad();
    pick.refuse_output(true);
    pick.fill(st);
    out.finish();
    st->stream_bytes = out.stream_bytes(); st->compressed_bytes = out.compressed_bytes();
    st->ms_deflate = out.ms_deflate();
    if (stream_stats) *stream_stats = out.stats();
}

// Text bytes per piece of sbx_view_sam: 64 MiB (not tuned), or SBX_SAM_PIECE_BYTES (tests: a decimal number of at least 1; anything
// else counts as unset).  Pieces are cut at line ends and written in order, so the value does not change a byte of the output.
uint64_t sam_piece_bytes() { return env_size("SBX_SAM_PIECE_BYTES", 64ull << 20); }

// The text of a set of entries (sbx_view_sam): measure() runs K13a, the offsets of the lines and the cut into pieces, and throws when
// a record is malformed -- nothing has been written by then --; emit() runs K13b piece by piece through two device and two pinned
// buffers, so that the copy and the write of a piece overlap the kernel of the next.  The resident sink calls the pair once over all
// entries, the streamed sink once per batch: the buffers are kept, the figures add up.
struct SamText {
    uint64_t budget = sam_piece_bytes();
    uint64_t text_bytes = 0;
    uint32_t n_pieces = 0;
    double ms = 0;                                      // device time of K13a, the offsets and K13b
    DevBuf<uint32_t> d_line_len, d_n_pieces, d_first;
    DevBuf<uint64_t> d_group, d_line_off, d_first_off;
    DevBuf<unsigned long long> d_acc;
    std::vector<uint32_t> first;
    std::vector<uint64_t> first_off;
    uint32_t pieces = 0;                                // of the entries measured last
    DevBuf<uint8_t> d_piece[2];
    PinnedBuf<uint8_t> h_piece[2];
    PinnedBuf<unsigned long long> h_acc;
    EventTimer t_a, t_b[2];
    Event ev_copy[2];
    Stream copy;

    void measure(const SamEntries& e, hipStream_t s) {
        const uint64_t n = e.n;
        const uint32_t groups = group_count(n);
        d_line_len.ensure((size_t)n + 2); d_n_pieces.ensure(1);
        d_group.ensure(groups + 2); d_line_off.ensure((size_t)n + 2);
        d_acc.ensure(kSamAccWords);
        SBX_HIP(hipMemsetAsync(d_acc.p, 0, kSamAccWords * sizeof(unsigned long long), s));
        t_a.start(s);
        launch_sam_measure(e, d_line_len.p, d_group.p, d_acc.p, s);
        if (n) {
            launch_scan64(d_group.p, groups, 0, s);
            launch_group_offsets(d_line_len.p, d_group.p, n, 0, d_line_off.p, s);
        }
        t_a.stop(s);
        launch_sam_pieces(d_line_off.p, n, budget, nullptr, nullptr, d_n_pieces.p, s);
        unsigned long long acc[kSamAccWords] = {0};
        pieces = 0;
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(&pieces, d_n_pieces.p, 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        if (acc[kSamAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kSamAccBad]));
        if (acc[kSamAccTooLong]) throw Error(SBX_EUNSUPPORTED, "a SAM line of 4 GiB or more");
        if (n) ms += t_a.ms();
        d_first.ensure((size_t)pieces + 2);
        d_first_off.ensure((size_t)pieces + 2);
        first.assign((size_t)pieces + 1, 0);
        first_off.assign((size_t)pieces + 1, 0);
        launch_sam_pieces(d_line_off.p, n, budget, d_first.p, d_first_off.p, d_n_pieces.p, s);
        SBX_HIP(hipMemcpyAsync(first.data(), d_first.p, first.size() * 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(first_off.data(), d_first_off.p, first_off.size() * 8, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
    }
    // the entries measure() saw, into f; returns when the last piece is written (the entries' bytes may then be overwritten)
    void emit(const SamEntries& e, hipStream_t s, OutputFile& f) {
        uint64_t max_piece = 0;
        for (uint32_t k = 0; k < pieces; ++k) max_piece = std::max(max_piece, first_off[k + 1] - first_off[k]);
        h_acc.ensure(2 * kSamAccWords);
        for (int b = 0; b < 2 && b < (int)pieces; ++b) { d_piece[b].ensure((size_t)max_piece + 64); h_piece[b].ensure((size_t)max_piece + 64); }
        if (!copy.get()) copy.create();
        try {
            auto finish = [&](uint32_t k) {             // piece k: its copy has arrived; check, write
                const int b = (int)(k & 1u);
                SBX_HIP(hipEventSynchronize(ev_copy[b].get()));
                ms += t_b[b].ms();
                if (h_acc.p[b * kSamAccWords + kSamAccOverrun])
                    throw Error(SBX_EFORMAT, "internal error: a SAM line did not have the length it was measured with");
                const size_t bytes = (size_t)(first_off[k + 1] - first_off[k]);
                f.write(h_piece[b].p, bytes);
            };
            for (uint32_t k = 0; k < pieces; ++k) {
                const int b = (int)(k & 1u);
                t_b[b].start(s);
                launch_sam_emit(e, d_line_len.p, d_line_off.p, first[k], first[k + 1], d_piece[b].p, d_acc.p, s);
                t_b[b].stop(s);
                if (k) finish(k - 1);
                SBX_HIP(hipStreamWaitEvent(copy.get(), t_b[b].b, 0));
                SBX_HIP(hipMemcpyAsync(h_piece[b].p, d_piece[b].p, (size_t)(first_off[k + 1] - first_off[k]), hipMemcpyDeviceToHost, copy.get()));
                SBX_HIP(hipMemcpyAsync(h_acc.p + b * kSamAccWords, d_acc.p, kSamAccWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, copy.get()));
                SBX_HIP(hipEventRecord(ev_copy[b].get(), copy.get()));
            }
            if (pieces) finish(pieces - 1);
        } catch (...) {                                 // (the pinned buffers may die with the caller's scope: nothing may still be copying into them)
            (void)hipStreamSynchronize(s);
            (void)hipStreamSynchronize(copy.get());
            throw;
        }
        if (e.n) text_bytes += first_off[pieces];
        n_pieces += pieces;
    }
};


// ---- the streamed SAM sink: no store and no new kernel; per batch K12a, K12b with offsets into U, K13a, the offsets, K13b ----
void view_sam_streamed(ViewJob& job, sbx_view_stats* st, sbx_stream_stats* stream_stats) {
    sbx_ctx* c = job.c.get();
    SamText sam;
    // next to a batch: 34 bytes per record of it (count, off, len, perm, line length and offset, the mask of -v) and the two device
    // pieces of the text -- no encoder and no window
    const uint64_t pieces = 2 * std::min<uint64_t>(sam.budget, 4 * record_bytes_max(c, job.rd) + (1ull << 20)) + (8ull << 20);
    const StreamBudget budget(pieces, 34, "selecting records of", "34 bytes per record of it and two pieces of text", iview_hint(job.rd));
    hipStream_t s = c->stream.get();
    DeviceRefNames names;
    upload_ref_names(c->hdr.refs, s, &names);
    SelectStep pick(job, SelectWants{true, true, true}, s);
    DevBuf<uint64_t> d_off;
    DevBuf<uint32_t> d_len, d_perm;
    OutputFile f(job.out_file);                         // the output is armed from here to the end
    f.write(job.text.data(), job.text.size());
    EventTimer t_b;
    read_batches(c, job.rd, budget.batch_u, &pick.n_batches, &pick.inflated, [&](const ViewBatch& vb) -> bool {
        if (!pick.run(vb, nullptr, s)) return false;
        const uint64_t n_sel = pick.books.acc[kViewAccRecords] - pick.before[kViewAccRecords];
        if (!n_sel) return true;
        // K12b with batch-local ordinals and offsets of U: the batch is the store
        d_off.ensure((size_t)n_sel + 2); d_len.ensure((size_t)n_sel + 2); d_perm.ensure((size_t)n_sel + 2);
        ViewEmitArgs b{};
        b.s = pick.a;
        b.group_entry_base = pick.d_group_entry_base.p; b.group_record_base = pick.d_group_record_base.p;
        b.store_delta = 0;
        b.record_base = 0; b.entry_base = 0;
        b.off = d_off.p; b.len = d_len.p;
        t_b.start(s);
        launch_view_emit(b, s);
        launch_iota(d_perm.p, n_sel, s);
        t_b.stop(s);
        const SamEntries e{c->U(), d_off.p, d_len.p, d_perm.p, n_sel, samc::RefNames{names.off.p, names.bytes.p, names.n()}};
        sam.measure(e, s);          // (a malformed selected record of this batch: earlier batches are written by now)
        st->ms_emit += t_b.ms();
        // (the next batch's K1 / K2 overwrite U and the descriptors: emit returns when K13b has read them)
        sam.emit(e, s, f);
        return true;
    });
    pick.refuse_bad();
    pick.refuse_output(true);
    pick.fill(st);
    f.finish(false);
    st->stream_bytes = sam.text_bytes;
    st->ms_gather = sam.ms;
    // the text has no window of its own: what is handed to the file is a piece of text
    sbx_stream_stats ss{};
    ss.n_windows = sam.n_pieces; ss.window_bytes = sam.budget;
    if (getenv("SBX_TIMING")) {
        fprintf(stderr, "[sbx] output: text_bytes=%llu n_pieces=%u piece_bytes=%llu\n", (unsigned long long)st->stream_bytes, sam.n_pieces,
                (unsigned long long)sam.budget);
        fprintf(stderr, "[sbx] stream: n_windows=%u window_bytes=%llu n_pack_launches=%llu ms_pack=%.3f\n", ss.n_windows,
                (unsigned long long)ss.window_bytes, (unsigned long long)ss.n_pack_launches, ss.ms_pack);
    }
    if (stream_stats) *stream_stats = ss;
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

}  // extern "C"

namespace {

// ---- the three sinks: the bodies behind sbx_view_run.  q: the validated request ----
int view_count(const sbx_view_request& q, int index_mode, sbx_view_index_stats* ix, uint64_t* count, sbx_view_stats* stats, char* err,
               size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!q.in_path || !count) throw Error(SBX_EINVAL, "null argument");
        ViewJob job(q);
        job.open(index_mode, false, ix);
        hipStream_t s = job.c->stream.get();
        SelectStep pick(job, SelectWants{false, false, false}, s);
        read_batches(job.c.get(), job.rd, index_batch_bytes(), &pick.n_batches, &pick.inflated, [&](const ViewBatch& vb) -> bool {
            pick.run(vb, nullptr, s);
            return true;                // (nothing is written: the pass goes on, and the refusal counts the bad records of the whole file)
        });
        pick.refuse_bad();
        sbx_view_stats st{};
        pick.fill(&st);
        *count = st.n_entries_out;
        job.finish(st, "count", stats);
    });
}

int view_bam(const sbx_view_request& q, int index_mode, sbx_view_index_stats* ix, sbx_view_stats* stats, sbx_stream_stats* stream_stats,
             char* err, size_t errlen) {
    const int rc = run_entry(err, errlen, [&] {
        if (!q.in_path) throw Error(SBX_EINVAL, "null argument");
        ViewJob job(q);
        check_level(q.level);
        if (job.to_stdout && q.with_index) throw Error(SBX_EINVAL, "an output on stdout cannot be indexed");
        if (!job.to_stdout) refuse_overwrite(q.in_path, job.path);
        job.open(index_mode, true, ix);
        const std::vector<uint8_t> header = bam_header_bytes(job.text, job.c->hdr.refs);
        sbx_view_stats st{};
        const uint64_t hook = stream_window_hook();
        const std::optional<StorePlan> fits = job.plan_store(header.size(), 48, hook);
        if (!fits) {
            view_bam_streamed(job, header, hook, &st, stream_stats);
            job.out_file.disarm();
            job.finish(st, "bam", stats);
            return;
        }
        SelectedRecords r;
        select_resident(job, *fits, &r, &st);
        DevBuf<uint64_t> d_out_off((size_t)r.n + 2);
        const WrittenBam w = write_store_output(job.out_file, header, r.store.p, r.off.p, r.len, r.perm.p, r.n, d_out_off.p, q.level,
                                                &r.record_bytes, "selected records", r.stream.get(), &st.ms_gather);
        job.out_file.disarm();
        st.stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.ms_deflate = w.ms_deflate;
        job.finish(st, "bam", stats);
    });
    // (the index is a pass of its own and not part of the figures)
    return rc != SBX_OK ? rc : index_written_bam(ViewJob::path_of(q), q.with_index, q.device, err, errlen);
}

int view_sam(const sbx_view_request& q, int index_mode, sbx_view_index_stats* ix, sbx_view_stats* stats, sbx_stream_stats* stream_stats,
             char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!q.in_path) throw Error(SBX_EINVAL, "null argument");
        ViewJob job(q);
        if (!job.to_stdout) refuse_overwrite(q.in_path, job.path);
        job.open(index_mode, q.with_header != 0, ix);
        sbx_view_stats st{};
        const std::optional<StorePlan> fits = job.plan_store(job.text.size(), 48 + 12, stream_window_hook());      // (+ length and offset of every line)
        if (!fits) {
            view_sam_streamed(job, &st, stream_stats);
            job.out_file.disarm();
            job.finish(st, "sam", stats);
            return;
        }
        const std::vector<RefSeq> refs = job.c->hdr.refs;   // (select_resident lets go of the context)
        SelectedRecords r;
        select_resident(job, *fits, &r, &st);
        hipStream_t s = r.stream.get();
        DeviceRefNames names;
        upload_ref_names(refs, s, &names);
        const SamEntries e{r.store.p, r.off.p, r.len.p, r.perm.p, r.n, samc::RefNames{names.off.p, names.bytes.p, names.n()}};

        // ---- K13a over all entries; then K13b piece by piece into the file, the header first ----
        SamText sam;
        sam.measure(e, s);                              // (a malformed selected record: SBX_EFORMAT before a byte is written)
        OutputFile f(job.out_file);
        f.write(job.text.data(), job.text.size());
        sam.emit(e, s, f);
        st.ms_gather += sam.ms;
        f.finish(false);
        job.out_file.disarm();
        st.stream_bytes = sam.text_bytes;
        job.finish(st, "sam", stats);
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] output: text_bytes=%llu n_pieces=%u piece_bytes=%llu\n", (unsigned long long)st.stream_bytes, sam.n_pieces,
                    (unsigned long long)sam.budget);
    });
}

sbx_view_request request_of(int sink, const char* in_path, const char* out_path, const sbx_filter* filter, const sbx_view_opts* opts,
                            const char* const* regions, size_t n_regions, const char* bed_path, const char* pg_command_line, int device) {
    sbx_view_request q{};
    q.struct_size = (uint32_t)sizeof q;
    q.sink = sink;
    q.in_path = in_path; q.out_path = out_path; q.filter = filter; q.opts = opts;
    q.regions = regions; q.n_regions = n_regions; q.bed_path = bed_path; q.pg_command_line = pg_command_line;
    q.level = -1; q.device = device;
    return q;
}

}  // namespace

extern "C" {

int sbx_view_run_streamed(const sbx_view_request* request, int index_mode, uint64_t* count, sbx_view_stats* stats, sbx_view_index_stats* ix,
                          sbx_stream_stats* stream_stats, char* err, size_t errlen) {
    if (stream_stats) *stream_stats = sbx_stream_stats{};
    sbx_view_request q{};
    const int rc = run_entry(err, errlen, [&] {
        if (!request) throw Error(SBX_EINVAL, "null argument");
        if (request->struct_size < offsetof(sbx_view_request, valid_only))
            throw Error(SBX_EINVAL, "sbx_view_request: struct_size " + std::to_string(request->struct_size) + " is smaller than the first version of the struct");
        memcpy(&q, request, std::min<size_t>(request->struct_size, sizeof q));      // (what the caller's struct lacks stays 0)
        if (q.sink != SBX_VIEW_SINK_COUNT && q.sink != SBX_VIEW_SINK_BAM && q.sink != SBX_VIEW_SINK_SAM)
            throw Error(SBX_EINVAL, "sbx_view_request: unknown sink " + std::to_string(q.sink));
    });
    if (rc != SBX_OK) return rc;
    if (q.sink == SBX_VIEW_SINK_COUNT) return view_count(q, index_mode, ix, count, stats, err, errlen);
    if (q.sink == SBX_VIEW_SINK_BAM) return view_bam(q, index_mode, ix, stats, stream_stats, err, errlen);
    return view_sam(q, index_mode, ix, stats, stream_stats, err, errlen);
}

int sbx_view_run_indexed(const sbx_view_request* request, int index_mode, uint64_t* count, sbx_view_stats* stats, sbx_view_index_stats* ix,
                         char* err, size_t errlen) {
    return sbx_view_run_streamed(request, index_mode, count, stats, ix, nullptr, err, errlen);
}

int sbx_view_run(const sbx_view_request* request, uint64_t* count, sbx_view_stats* stats, char* err, size_t errlen) {
    return sbx_view_run_indexed(request, SBX_VIEW_INDEX_OFF, count, stats, nullptr, err, errlen);
}

// the three entry points of before sbx_view_run: the same call with valid_only = 0
int sbx_view_count(const char* in_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions, size_t n_regions,
                   const char* bed_path, int device, uint64_t* count, sbx_view_stats* stats, char* err, size_t errlen) {
    const sbx_view_request q = request_of(SBX_VIEW_SINK_COUNT, in_path, nullptr, filter, opts, regions, n_regions, bed_path, nullptr, device);
    return sbx_view_run(&q, count, stats, err, errlen);
}

int sbx_view_bam(const char* in_path, const char* out_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions,
                 size_t n_regions, const char* bed_path, const char* pg_command_line, int level, int with_index, int device,
                 sbx_view_stats* stats, char* err, size_t errlen) {
    sbx_view_request q = request_of(SBX_VIEW_SINK_BAM, in_path, out_path, filter, opts, regions, n_regions, bed_path, pg_command_line, device);
    q.level = level; q.with_index = with_index;
    return sbx_view_run(&q, nullptr, stats, err, errlen);
}

int sbx_view_sam(const char* in_path, const char* out_path, const sbx_filter* filter, const sbx_view_opts* opts, const char* const* regions,
                 size_t n_regions, const char* bed_path, const char* pg_command_line, int with_header, int device, sbx_view_stats* stats,
                 char* err, size_t errlen) {
    sbx_view_request q = request_of(SBX_VIEW_SINK_SAM, in_path, out_path, filter, opts, regions, n_regions, bed_path, pg_command_line, device);
    q.with_header = with_header;
    return sbx_view_run(&q, nullptr, stats, err, errlen);
}

}  // extern "C"
