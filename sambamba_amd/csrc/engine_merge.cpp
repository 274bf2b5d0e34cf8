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
//
// Inputs whose records do not fit the device next to one batch of the read pass take the WINDOWED path (merge_windowed; also forced
// by SBX_MERGE_WINDOW_BYTES): no record store.  The key pass is the same loop over the inputs with the same batch step
// (MergePass::step) -- K9a, or K11a and the key-only emit; nothing is copied -- and saves every input's batches; K9b sorts the keys
// of all records; the offsets of the merged stream become one destination per record (K9d-1) and one span of destinations per
// (input, batch) (K9d-2); then, for every window of whole pieces of the stream, the inputs that have a batch whose span meets the
// window are opened again in input order, one at a time, those batches go through K1 + K2 once more, and K9d-3 (an input nothing
// changes in) or K11a + K11c (a rewritten one) put the records' bytes in place.  The loop over windows, inputs and batches, the
// choice of the window and the two consistency checks are engine_windows.hpp, shared with sort and markdup.  The file is the
// resident path's byte for byte.  Coordinate-sorted inputs go to ascending, disjoint stretches of the output, batch by batch, so
// every input is inflated about twice in all.
#include "engine_windows.hpp"
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
    // the file as the key pass of the windowed path found it: what a later open for a window must find again
    uint64_t seen_blocks = 0, seen_u_total = 0, seen_first_record = 0;
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

// the tables K11 needs of one input, on the device
struct InputTables {
    DevBuf<int32_t> ref_map;
    DevBuf<RenameEntry> entries;
    DevBuf<char> blob;
    void upload(const MergeInput& in, const std::vector<int32_t>& map) {
        ref_map.alloc(map.size() + 1); entries.alloc(in.entries.size() + 1); blob.alloc(in.blob.size() + 1);
        if (!map.empty()) SBX_HIP(hipMemcpy(ref_map.p, map.data(), map.size() * 4, hipMemcpyHostToDevice));
        if (!in.entries.empty()) {
            SBX_HIP(hipMemcpy(entries.p, in.entries.data(), in.entries.size() * sizeof(RenameEntry), hipMemcpyHostToDevice));
            SBX_HIP(hipMemcpy(blob.p, in.blob.data(), in.blob.size(), hipMemcpyHostToDevice));
        }
    }
};

// K11's scratch, per batch
struct MergeScratch {
    DevBuf<uint32_t> new_len, keep, patch_at, patch_entry;
    DevBuf<uint64_t> key, len_base, keep_base, tile_sum;
    static constexpr uint64_t kPerRecord = 4 + 4 + 8 + 8 + 8 + 8 + 8;
    MergeBatch batch(uint64_t nrec) {
        const size_t m = (size_t)nrec + 2;
        new_len.ensure(m); keep.ensure(m); key.ensure(m); patch_at.ensure(2 * m); patch_entry.ensure(2 * m);
        len_base.ensure(m); keep_base.ensure(m); tile_sum.ensure(len_tiles(nrec) + 2);
        return MergeBatch{new_len.p, keep.p, key.p, patch_at.p, patch_entry.p, len_base.p, keep_base.p, tile_sum.p};
    }
    void release() {
        new_len.release(); keep.release(); key.release(); patch_at.release(); patch_entry.release();
        len_base.release(); keep_base.release(); tile_sum.release();
    }
};

// the arguments of K11 for a batch of input `in` as it lies in the context
MergeArgs merge_args(sbx_ctx* c, const MergeInput& in, const InputTables& tab, int32_t n_ref_merged, bool use_filter, uint64_t nrec,
                     uint64_t base, uint64_t next, const MergeBatch& b, unsigned long long* d_acc) {
    MergeArgs a{};
    a.U = c->U(); a.desc = c->d_desc.p; a.n = nrec; a.u_end = next - base;
    a.n_ref_own = in.n_ref; a.n_ref_merged = n_ref_merged; a.ref_map = tab.ref_map.p;
    a.table = RenameTable{tab.entries.p, tab.blob.p, (uint32_t)in.entries.size()};
    a.use_filter = use_filter ? 1u : 0u;
    a.b = b;
    a.acc = d_acc;
    return a;
}

// The read pass of both paths: key, length and -- with a store -- offset of every record that takes part, numbered input by input,
// and the one batch step around K9a (an input nothing changes in) or K11 (a rewritten one).
struct MergePass {
    int32_t n_ref;                  // of the merged dictionary
    bool use_filter;
    uint8_t* store;                 // the resident record store, or null: nothing is copied and no offset kept (the windowed path)
    uint64_t capacity;
    DevBuf<uint64_t> d_key, d_off, d_group_base;
    DevBuf<uint32_t> d_len, d_group_count;
    DevBuf<unsigned long long> d_acc{kMergeAccWords};
    unsigned long long acc[kMergeAccWords] = {0ull, ~0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    MergeScratch scratch;
    EventTimer t_k;
    uint64_t n_in = 0, n_kept = 0, store_at = 0, k11_new_bytes = 0;
    bool too_many = false, store_full = false;

    MergePass(int32_t n_ref_, bool use_filter_, uint8_t* store_, uint64_t capacity_)
        : n_ref(n_ref_), use_filter(use_filter_), store(store_), capacity(capacity_) {
        SBX_HIP(hipMemcpy(d_acc.p, acc, sizeof acc, hipMemcpyHostToDevice));
    }
    // One batch of for_each_record_batch over input `in`; cur: the inflated offset of the input behind its batches so far.  Returns
    // false when the pass has to stop (too_many, store_full or acc[kSortAccBad] say why).
    bool step(sbx_ctx* c, const MergeInput& in, const InputTables& tab, bool fast, uint64_t nrec, uint64_t base, uint64_t next, uint64_t* cur,
              sbx_merge_stats* st) {
        hipStream_t s = c->stream.get();
        if (n_kept + nrec > 0xFFFFFFF0ull) { too_many = true; return false; }
        const size_t want = (size_t)(n_kept + nrec + 2);
        grow_keeping(d_key, (size_t)n_kept, want, s);
        if (store) grow_keeping(d_off, (size_t)n_kept, want, s);
        grow_keeping(d_len, (size_t)n_kept, want, s);
        if (fast) {
            if (store && store_at + (next - *cur) > capacity) { store_full = true; return false; }
            if (use_filter) { d_group_count.ensure(sort_keys_groups(nrec) + 4); d_group_base.ensure(sort_keys_groups(nrec) + 4); }
            t_k.start(s);
            if (store && next > *cur) SBX_HIP(hipMemcpyAsync(store + store_at, c->U() + (*cur - base), next - *cur, hipMemcpyDeviceToDevice, s));
            SortKeysArgs a{};
            a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = next - base;
            a.n_ref = in.n_ref; a.key_n_ref = n_ref; a.use_filter = use_filter ? 1u : 0u;
            a.store_delta = store ? (int64_t)store_at + (int64_t)base - (int64_t)*cur : 0;
            a.out_base = n_kept;
            a.key = d_key.p; a.off = store ? d_off.p : nullptr; a.len = d_len.p; a.acc = d_acc.p;
            launch_sort_keys(a, d_group_count.p, d_group_base.p, s);
            t_k.stop(s);
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            if (store) store_at += next - *cur;
        } else {
            MergeArgs a = merge_args(c, in, tab, n_ref, use_filter, nrec, base, next, scratch.batch(nrec), d_acc.p);
            a.store = store; a.store_at = store_at; a.out_base = n_kept;
            a.key = d_key.p; a.off = d_off.p; a.len = d_len.p;
            const unsigned long long bytes_before = acc[kSortAccBytes];
            uint64_t batch_bytes = 0;
            t_k.start(s);
            launch_merge_describe(a, s);
            SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
            if (nrec) SBX_HIP(hipMemcpyAsync(&batch_bytes, scratch.len_base.p + nrec, 8, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            // the scanned size of the batch against what is left of the store, before a byte is written
            if (store && !acc[kSortAccBad] && store_at + batch_bytes > capacity) store_full = true;
            // (without a store: the key-only emit)
            if (!acc[kSortAccBad] && !store_full) launch_merge_rewrite(a, s);
            t_k.stop(s);
            SBX_HIP(hipStreamSynchronize(s));
            if (store_full) return false;
            k11_new_bytes += acc[kSortAccBytes] - bytes_before;
            if (store) store_at += batch_bytes;
        }
        // (the next batch's K1 / K2 overwrite U and the descriptors: the kernels above and the copy have ended)
        st->ms_inflate += c->stats.ms_inflate; st->ms_index += c->stats.ms_index; st->ms_rewrite += t_k.ms();
        n_in += nrec;
        n_kept = acc[kSortAccKept];
        *cur = next;
        return acc[kSortAccBad] == 0;
    }
    // behind the batches of input `path`
    void refuse(const char* path) const {
        if (too_many) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records");
        if (store_full) throw Error(SBX_ENOMEM, std::string("the record store is full at input ") + path);
        if (acc[kSortAccBad]) throw Error(SBX_EFORMAT, malformed_records_message(acc[kSortAccBad], path));
    }
    void check_counts() const {
        if (!use_filter && n_kept != n_in)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_kept) + " of " + std::to_string(n_in) + " records received a key");
    }
};

void print_merge_line(const sbx_merge_stats& st, double headers_ms, double read_ms, double sort_ms, double write_ms) {
    fprintf(stderr, "[sbx] merge: n_inputs=%u n_records_in=%llu n_records_out=%llu n_records_rewritten=%llu bytes_grown=%lld "
                    "inflated_bytes=%llu merged_stream_bytes=%llu compressed_bytes=%llu key_bits=%u n_sort_passes=%u n_batches=%u "
                    "ms_inflate=%.2f ms_index=%.2f ms_rewrite=%.2f ms_sort=%.2f ms_gather=%.2f ms_deflate=%.2f ms_total_wall=%.1f "
                    "(headers %.1f, read passes %.1f, sort %.1f, write %.1f)\n",
            st.n_inputs, (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_out,
            (unsigned long long)st.n_records_rewritten, (long long)st.bytes_grown, (unsigned long long)st.inflated_bytes,
            (unsigned long long)st.merged_stream_bytes, (unsigned long long)st.compressed_bytes, st.key_bits, st.n_sort_passes, st.n_batches,
            st.ms_inflate, st.ms_index, st.ms_rewrite, st.ms_sort, st.ms_gather, st.ms_deflate, st.ms_total_wall, headers_ms, read_ms, sort_ms, write_ms);
}

// SBX_MERGE_WINDOW_BYTES (tests, measurements): forces the windowed path with windows of this many bytes, rounded up to whole pieces.
// 0: unset (or not a positive decimal number).
uint64_t merge_window_hook() { return env_u64("SBX_MERGE_WINDOW_BYTES").value_or(0); }

constexpr uint64_t kWindowedPerRecord = 36;     // bytes per record while the keys are sorted (as engine_sort.cpp): key, key2, len, val, val2, dest / out_off

// what both paths know when the headers are merged
struct MergeJob {
    const char* const* in_paths;
    int device;
    const sbx_filter* filter;
    bool use_filter, force_rewrite;
    std::vector<MergeInput> in;
    mergec::MergedHeader mh;
    std::vector<uint8_t> header;
    uint64_t u_sum = 0;
    int32_t n_ref() const { return (int32_t)mh.refs.size(); }
    bool fast(size_t k) const { return in[k].identity && !force_rewrite; }
};

// An input opened again for a window must be the file the key pass read: the saved batches index its block table.  The same
// number of blocks, inflated bytes and first-record offset, or SBX_EIO before anything of the file goes to the device.
void note_input(const sbx_ctx* c, MergeInput* in) {
    in->seen_blocks = c->blocks.size(); in->seen_u_total = c->blocks.out_off.back(); in->seen_first_record = c->hdr.first_record_off;
}
void refuse_changed_input(const sbx_ctx* c, const MergeInput& in) {
    if (c->blocks.size() != in.seen_blocks || c->blocks.out_off.back() != in.seen_u_total || c->hdr.first_record_off != in.seen_first_record)
        throw Error(SBX_EIO, sortc::batch_refusal(sortc::kMergeWindowWords));
}

// The merge of inputs whose records do not stay on the device (or SBX_MERGE_WINDOW_BYTES); see the head of this file.
void merge_windowed(MergeJob& job, OutputGuard& out_file, int level, uint64_t hook, double w0, sbx_merge_stats* stats,
                    sbx_merge_window_stats* window_stats) {
    const std::vector<uint8_t>& header = job.header;
    const uint64_t hlen = header.size();
    const size_t n_in_files = job.in.size();
    const int32_t n_ref = job.n_ref();
    const bool use_filter = job.use_filter;
    uint64_t record_bytes = 0;
    for (const MergeInput& in : job.in) record_bytes += in.u_total - in.u_first;
    WindowBudget budget(job.u_sum, 0, record_bytes, hlen, sortc::kMergeWindowWords, hook);
    const uint64_t keys_est = budget.est_records * kWindowedPerRecord;
    const uint64_t scratch_est = ((WindowBudget::kMinBatch / 5) / 160 + 4096) * MergeScratch::kPerRecord;
    budget.fit(keys_est + scratch_est,
               std::to_string(keys_est) + " for the keys of the records, " + std::to_string(scratch_est) + " for K11's scratch of one batch, " +
                   std::to_string(WindowBudget::kMinBatch) + " for one read batch, " + std::to_string(budget.out_reserve) +
                   " for the encoder and " + std::to_string(budget.cap_bytes) + " for a window of one piece");
    MergePass pass(n_ref, use_filter, nullptr, 0);
    const unsigned long long* acc = pass.acc;
    std::vector<InputTables> tables(n_in_files);
    for (size_t k = 0; k < n_in_files; ++k)
        if (!job.fast(k)) tables[k].upload(job.in[k], job.mh.maps[k].ref);
    const double w1 = wall_now();

    // ---- the key pass: every input in turn, nothing copied; the batches are saved ----
    sbx_merge_stats st{};
    std::vector<std::vector<SavedBatch>> saved(n_in_files);
    std::vector<WindowSource> sources(n_in_files);
    Standalone open_input;                              // the one input that is open
    uint32_t n_batches = 0;
    for (size_t k = 0; k < n_in_files; ++k) {
        open_input = open_record_pass(job.in_paths[k], job.device, job.filter, use_filter);
        sbx_ctx* c = open_input.get();
        note_input(c, &job.in[k]);
        uint64_t cur = job.in[k].u_first;
        uint32_t nb = 0;
        sources[k].first_ordinal = pass.n_kept;
        for_each_record_batch(c, budget.batch_u, &nb, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            const uint64_t before = pass.n_kept;
            const bool go_on = pass.step(c, job.in[k], tables[k], job.fast(k), nrec, base, next, &cur, &st);
            saved[k].back().first_kept = before;
            saved[k].back().n_kept = pass.n_kept - before;
            return go_on;
        }, &saved[k]);
        n_batches += nb;
        open_input.reset();                             // one context at a time
        pass.refuse(job.in_paths[k]);
        sources[k].n_ordinals = pass.n_kept - sources[k].first_ordinal;
        sources[k].saved = &saved[k];
        sources[k].open = [&open_input, &job, k] {
            open_input = open_record_pass(job.in_paths[k], job.device, job.filter, job.use_filter);
            refuse_changed_input(open_input.get(), job.in[k]);
            return open_input.get();
        };
        sources[k].close = [&open_input] { open_input.reset(); };
    }
    pass.check_counts();
    const uint64_t n_in = pass.n_in, n = pass.n_kept;
    const double w2 = wall_now();

    // ---- K9b over all keys, the offsets, K9d-1 and K9d-2 ----
    Stream stream;
    stream.create();
    hipStream_t s = stream.get();
    double ms_dest = 0;
    DevBuf<uint64_t> d_dest((size_t)n + 2);
    BatchSpans spans;
    uint64_t total = hlen;
    {
        ResidentOrder order;
        sort_resident(pass.d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
        st.ms_sort = order.ms_sort;
        st.key_bits = order.key_bits; st.n_sort_passes = order.n_passes;
        const OutputPlan plan = plan_output(pass.d_len.p, order.perm, n, hlen, order.key2.p, s, &st.ms_gather);
        total = plan.total;
        if (total != hlen + acc[kSortAccBytes]) throw Error(SBX_EFORMAT, "internal error: the offsets of the merged records do not add up");
        spans.upload(sources, n, s);
        EventTimer t;
        t.start(s);
        launch_window_dest(order.perm, order.key2.p, n, d_dest.p, s);
        spans.launch(d_dest.p, pass.d_len.p, s);
        t.stop(s);
        spans.read_back(s);
        ms_dest = t.ms();
        // keys, key2, val / val2 and the offsets go before the first window comes (order: end of this scope)
        pass.d_key.release();
    }

    // ---- the windows: K9d-3 or K11a + K11c for every saved batch that meets one ----
    // No input is open now: the batch buffers of the one the windows open count against the window.  They follow the largest batch
    // that was saved (a record longer than batch_u doubles its batch): about five times its inflated bytes (index_batch_bytes), taken
    // as six here, plus the tables of the context.  The factor is NOT measured on inputs that need the path.
    uint64_t largest_batch = 0;
    for (const std::vector<SavedBatch>& sv : saved)
        for (const SavedBatch& sb : sv) largest_batch = std::max<uint64_t>(largest_batch, sb.run.ue - sb.base);
    budget.batch_reserve = 6 * largest_batch + (256ull << 20);
    DevBuf<uint32_t> d_rank;
    DevBuf<unsigned long long> d_acc_replay(kMergeAccWords);       // K11a counts again when a batch is replayed: not into the call's figures
    SBX_HIP(hipMemset(d_acc_replay.p, 0, kMergeAccWords * sizeof(unsigned long long)));
    const WindowedOutput w = write_windows(sources, s, out_file, header, total, budget, spans, level, [&](size_t k, sbx_ctx* c, const SavedBatch& sb,
                                           const RecordBatch& rb, const sortc::Window& win, uint8_t* d_win, unsigned long long* d_wacc, hipStream_t ws) {
        if (job.fast(k)) {
            if (use_filter) {
                pass.d_group_count.ensure(sort_keys_groups(rb.nrec) + 4);
                pass.d_group_base.ensure(sort_keys_groups(rb.nrec) + 4);
                d_rank.ensure((size_t)rb.nrec + 2);
            }
            WindowScatterArgs a{};
            a.U = c->U(); a.desc = c->d_desc.p; a.n = rb.nrec; a.u_end = rb.next - rb.base; a.use_filter = use_filter ? 1u : 0u;
            a.first_kept = sb.first_kept; a.n_kept = sb.n_kept;
            a.dest = d_dest.p; a.len = pass.d_len.p; a.w0 = win.w0; a.w1 = win.w1; a.window = d_win; a.acc = d_wacc;
            launch_window_scatter(a, pass.d_group_count.p, pass.d_group_base.p, d_rank.p, ws);
            return;
        }
        const MergeArgs a = merge_args(c, job.in[k], tables[k], n_ref, use_filter, rb.nrec, rb.base, rb.next, pass.scratch.batch(rb.nrec), d_acc_replay.p);
        MergeWindowArgs mw{};
        mw.first_kept = sb.first_kept; mw.n_kept = sb.n_kept;
        mw.dest = d_dest.p; mw.len = pass.d_len.p; mw.w0 = win.w0; mw.w1 = win.w1; mw.window = d_win; mw.acc = d_wacc;
        launch_merge_describe(a, ws);
        launch_merge_window_scatter(a, mw, ws);
    });
    out_file.disarm();
    const double w3 = w.w_planned, w4 = w.w_written;

    st.ms_gather += ms_dest + w.ms_scatter;
    st.n_records_in = n_in; st.n_records_out = n;
    st.n_records_rewritten = acc[kMergeAccRewritten];
    st.bytes_grown = (int64_t)pass.k11_new_bytes - (int64_t)acc[kMergeAccOldBytes];
    st.inflated_bytes = job.u_sum; st.merged_stream_bytes = total; st.compressed_bytes = w.compressed_bytes;
    st.n_inputs = (uint32_t)n_in_files; st.n_batches = n_batches;
    st.ms_deflate = w.ms_deflate;
    st.ms_total_wall = (w4 - w0) * 1e3;
    sbx_merge_window_stats ws{};
    ws.n_windows = w.n_windows; ws.n_batch_runs = (uint32_t)w.n_batch_runs; ws.n_batches_skipped = (uint32_t)w.n_batches_skipped;
    ws.n_input_opens = (uint32_t)w.n_input_opens; ws.window_bytes = w.span;
    ws.ms_dest = ms_dest; ws.ms_scatter = w.ms_scatter; ws.ms_inflate_replay = w.ms_inflate_replay; ws.ms_index_replay = w.ms_index_replay;
    if (getenv("SBX_TIMING")) {
        fprintf(stderr, "[sbx] merge-windows: n_windows=%u window_bytes=%llu n_batch_runs=%u n_batches_skipped=%u n_input_opens=%u ms_dest=%.2f "
                        "ms_scatter=%.2f ms_inflate_replay=%.2f ms_index_replay=%.2f\n", ws.n_windows, (unsigned long long)ws.window_bytes,
                ws.n_batch_runs, ws.n_batches_skipped, ws.n_input_opens, ws.ms_dest, ws.ms_scatter, ws.ms_inflate_replay, ws.ms_index_replay);
        print_merge_line(st, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
    }
    if (stats) *stats = st;
    if (window_stats) {
        ws.struct_size = window_stats->struct_size;
        memcpy(window_stats, &ws, sizeof ws);
    }
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

int sbx_merge_bam_run(const char* out_path, const char* const* in_paths, int n_inputs, const sbx_filter* filter, int level, int with_index,
                      int device, sbx_merge_stats* stats, sbx_merge_window_stats* window_stats, char* err, size_t errlen) {
    const int rc = run_entry(err, errlen, [&] {
        if (!out_path || !in_paths) throw Error(SBX_EINVAL, "null argument");
        if (window_stats) {
            if (window_stats->struct_size < sizeof(sbx_merge_window_stats))
                throw Error(SBX_EINVAL, "sbx_merge_window_stats: struct_size " + std::to_string(window_stats->struct_size) + " is smaller than the struct");
            const uint32_t size = window_stats->struct_size;                 // the resident path: everything else is 0
            memset(window_stats, 0, sizeof *window_stats);
            window_stats->struct_size = size;
        }
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
        MergeJob job;
        job.in_paths = in_paths; job.device = device; job.filter = filter; job.use_filter = use_filter;
        std::vector<MergeInput>& in = job.in;
        in.resize(n_in_files);
        std::vector<std::string> texts;
        for (size_t k = 0; k < n_in_files; ++k) {
            Standalone c = open_standalone(in_paths[k], device);
            in[k].text = text_with_sq_lines(c->hdr, in_paths[k]);
            in[k].u_total = c->blocks.out_off.back();
            in[k].u_first = std::min<uint64_t>(c->hdr.first_record_off, in[k].u_total);
            in[k].n_ref = (int32_t)c->hdr.refs.size();
            job.u_sum += in[k].u_total;
            texts.push_back(in[k].text);
        }
        mergec::MergedHeader& mh = job.mh;
        {
            std::string why;
            const int rc = mergec::merge_headers(texts, &mh, &why);
            if (rc != SBX_OK) throw Error(rc, why);
        }
        const int32_t n_ref = job.n_ref();
        job.header = bam_header_bytes(mh.text, mh.refs);
        const std::vector<uint8_t>& header = job.header;
        const uint64_t hlen = header.size();
        const uint64_t u_sum = job.u_sum;
        job.force_rewrite = getenv("SBX_MERGE_FORCE_REWRITE") && atoi(getenv("SBX_MERGE_FORCE_REWRITE")) != 0;

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
        // The records stay on the device when they fit; otherwise (or when the hook says so) the merged stream is written in windows.
        const uint64_t hook = merge_window_hook();
        std::optional<StorePlan> fits;
        if (!hook) fits = plan_if_fits([&] { return plan_store_bytes(capacity, hlen, 48, "merging", "the files do"); });   // (the device is the one the inputs were opened on)
        if (!fits) {
            merge_windowed(job, out_file, level, hook, w0, stats, window_stats);
            return;
        }
        const StorePlan& plan = *fits;
        DevBuf<uint8_t> d_store((size_t)capacity + 64);
        MergePass pass(n_ref, use_filter, d_store.p, capacity);
        const unsigned long long* acc = pass.acc;
        const double w1 = wall_now();

        // ---- the read passes ----
        sbx_merge_stats st{};
        uint32_t n_batches = 0;
        for (size_t k = 0; k < n_in_files; ++k) {
            Standalone c = open_record_pass(in_paths[k], device, filter, use_filter);
            InputTables tab;
            if (!job.fast(k)) tab.upload(in[k], mh.maps[k].ref);
            uint64_t cur = in[k].u_first;
            uint32_t nb = 0;
            for_each_record_batch(c.get(), plan.batch_u, &nb, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
                return pass.step(c.get(), in[k], tab, job.fast(k), nrec, base, next, &cur, &st);
            });
            n_batches += nb;
            c.reset();                                   // the batch buffers make room for the next input, the sort and the output pieces
            pass.refuse(in_paths[k]);
        }
        pass.check_counts();
        const uint64_t n_in = pass.n_in, n = pass.n_kept;
        pass.scratch.release();
        const double w2 = wall_now();

        // ---- K9b: the merge ----
        Stream stream;
        stream.create();
        hipStream_t s = stream.get();
        ResidentOrder order;
        sort_resident(pass.d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
        // the keys are done with: one of their buffers holds the output offsets
        pass.d_key.release();
        st.ms_sort = order.ms_sort;

        // ---- offsets, K9c + deflate, piece by piece ----
        const WrittenBam w = write_store_output(out_file, header, d_store.p, pass.d_off.p, pass.d_len, order.perm, n, order.key2.p, level,
                                                &acc[kSortAccBytes], "merged records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = w.w_planned, w4 = wall_now();
        st.n_records_in = n_in; st.n_records_out = n;
        st.n_records_rewritten = acc[kMergeAccRewritten];
        st.bytes_grown = (int64_t)pass.k11_new_bytes - (int64_t)acc[kMergeAccOldBytes];
        st.inflated_bytes = u_sum; st.merged_stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.n_inputs = (uint32_t)n_in_files; st.key_bits = order.key_bits; st.n_sort_passes = order.n_passes; st.n_batches = n_batches;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (w4 - w0) * 1e3;
        if (getenv("SBX_TIMING")) print_merge_line(st, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
        if (stats) *stats = st;
    });
    // (the index is a pass of its own and not part of the merge's figures)
    return rc != SBX_OK ? rc : index_written_bam(out_path, with_index, device, err, errlen);
}

int sbx_merge_bam(const char* out_path, const char* const* in_paths, int n_inputs, const sbx_filter* filter, int level, int with_index,
                  int device, sbx_merge_stats* stats, char* err, size_t errlen) {
    return sbx_merge_bam_run(out_path, in_paths, n_inputs, filter, level, with_index, device, stats, nullptr, err, errlen);
}

}  // extern "C"
