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
// sbx_markdup, sbx_merge_bam and sbx_view_bam.  KeyPass::step is the one batch step around K9a: both paths below call it.
//
// A file whose records do not fit the device next to one batch of the read pass takes the WINDOWED path (sort_file_windowed; also
// forced by SBX_SORT_WINDOW_BYTES): no record store.  The key pass runs K9a alone and saves its batches (for_each_record_batch with
// `saved`); K9b sorts the keys; the offsets of the sorted stream become one destination per record (K9d-1) and one span of
// destinations per batch (K9d-2); then, for every window of whole pieces of the stream that fits the device, the batches whose span
// meets the window are run again (run_record_batch: the same K1 + K2, the same U and descriptors) and K9d-3 scatters their records
// into the window, which goes through the same encoder to the file.  No temporary file and no merge; the file is the resident
// path's byte for byte.  The budget of device memory, the spans, the choice of the window and the loop over windows and batches are
// engine_windows.hpp, shared with sbx_markdup (whose output is in input order); what is here is the key pass, the order and the
// callback that launches K9d-3.  The name orders stay resident and refuse with
// SBX_ENOMEM what does not fit (sbx_merge_bam has a windowed path of its own, engine_merge.cpp); sbx_fixbins, sbx_import_sam and view in file order, BAM and SAM sink, stream it (engine_streamout.hpp).
//
// sbx_sort_bam_by_name (`sambamba sort -n / -N`, with or without -M) is the same call with another order: next to K9a, K14a
// (namesort.hip) builds the key of every kept record's name in a key store of 64-bit words, and the order is an LSD sort over those
// words -- the -M word first, then the words from the last to word 0, each one K14b + K9b, and only the words and bits that vary.
#include "engine_windows.hpp"
#include "namesort.hpp"
#include "sort_core.hpp"

namespace {

// The keys of the names while the batches arrive (K14a) and the order over them (K14b + K9b).
struct NameKeys {
    uint32_t order = 0;             // nsc::kOrderLex / kOrderNatural
    bool match_mates = false;
    DevBuf<uint64_t> store, off, mate;          // the key store, [n + 1] where a record's key starts in it, [n] the -M words
    DevBuf<uint32_t> words;                     // of one batch
    DevBuf<uint64_t> word_base;
    DevBuf<unsigned long long> d_acc;
    unsigned long long acc[kNameAccWords];
    uint64_t n_words = 0;                       // key words of the batches so far
    uint32_t words_sorted = 0;

    void init(uint32_t order_, bool match_mates_, hipStream_t s) {
        order = order_;
        match_mates = match_mates_;
        d_acc = DevBuf<unsigned long long>(kNameAccWords);
        name_acc_init(acc);
        SBX_HIP(hipMemcpyAsync(d_acc.p, acc, sizeof acc, hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));
    }
    // K14a over the kept records [first, first + n) of a batch (K9a has written their offsets and lengths, their bytes are queued
    // into the record store on the same stream).  Returns false when a name or an HI tag was refused.
    bool add_batch(const uint8_t* d_store, const uint64_t* d_off, const uint32_t* d_len, uint64_t first, uint64_t n, hipStream_t s,
                   double* ms_keys) {
        if (!n) return true;
        grow_keeping(off, (size_t)first, (size_t)(first + n + 2), s);       // (emit writes off[first] again)
        if (match_mates) grow_keeping(mate, (size_t)first, (size_t)(first + n + 2), s);
        words.ensure((size_t)n + 4);
        word_base.ensure((size_t)n + 4);
        NameKeyArgs a{};
        a.store = d_store; a.off = d_off; a.len = d_len; a.first = first; a.n = n;
        a.order = order; a.match_mates = match_mates ? 1u : 0u;
        a.words = words.p; a.word_base = word_base.p; a.key_base = n_words;
        a.key_off = off.p; a.mate_word = mate.p; a.acc = d_acc.p;
        EventTimer t;
        t.start(s);
        launch_name_key_measure(a, s);
        launch_count_scan(words.p, (uint32_t)n, word_base.p, s);
        t.stop(s);
        uint64_t batch_words = 0;
        SBX_HIP(hipMemcpyAsync(&batch_words, word_base.p + n, 8, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, 2 * sizeof acc[0], hipMemcpyDeviceToHost, s));      // the two counts of refusals
        SBX_HIP(hipStreamSynchronize(s));
        *ms_keys += t.ms();
        if (acc[kNameAccBadName] || acc[kNameAccBadHi]) return false;
        grow_keeping(store, (size_t)n_words, (size_t)(n_words + batch_words + 2), s);     // (SBX_ENOMEM when the keys do not fit)
        a.key_store = store.p;
        t.start(s);
        launch_name_key_emit(a, s);
        t.stop(s);
        *ms_keys += t.ms();
        n_words += batch_words;
        return true;
    }
    void refuse_bad() {
        if (!acc[kNameAccBadName] && !acc[kNameAccBadHi]) return;
        if (acc[kNameAccBadName])
            throw Error(SBX_EFORMAT, std::to_string(acc[kNameAccBadName]) + " record(s) have a read name that is not NUL-terminated inside the record or "
                                     "holds a byte outside 0x01..0x7F: such names are not sorted");
        throw Error(SBX_EFORMAT, std::to_string(acc[kNameAccBadHi]) + " record(s) have an HI tag that is not an integer fitting int, or aux fields that "
                                 "run past the record: -M cannot order them");
    }
    // LSD over the words: the -M word first, then the key words from the last to word 0; a word no bit of which varies costs nothing
    void sort(uint64_t* d_key, uint64_t n, hipStream_t s, ResidentOrder* o) {
        begin_resident_order(n, s, o);
        if (!n) return;
        SBX_HIP(hipMemcpyAsync(acc, d_acc.p, sizeof acc, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        EventTimer t;
        if (match_mates && (acc[kNameAccMateOr] ^ acc[kNameAccMateAnd])) {
            t.start(s);
            launch_name_mate_gather(mate.p, o->perm, n, d_key, s);
            t.stop(s);
            continue_resident_order(d_key, n, acc[kNameAccMateOr] ^ acc[kNameAccMateAnd], s, o);
            o->ms_sort += t.ms();
            ++words_sorted;
        }
        const uint32_t w_min = (uint32_t)std::min<unsigned long long>(acc[kNameAccMinWords], nsc::kMaxKeyWords);
        const uint32_t w_max = (uint32_t)std::min<unsigned long long>(acc[kNameAccMaxWords], nsc::kMaxKeyWords);
        for (uint32_t w = w_max; w-- > 0;) {
            // (from the shortest key on, some record has ended at this word and counts as 0)
            const uint64_t varying = acc[kNameAccOr + w] ^ (w < w_min ? acc[kNameAccAnd + w] : 0ull);
            if (!varying) continue;
            t.start(s);
            launch_name_word_gather(store.p, off.p, o->perm, n, w, d_key, s);
            t.stop(s);
            continue_resident_order(d_key, n, varying, s, o);
            o->ms_sort += t.ms();
            ++words_sorted;
        }
    }
    void release() { store.release(); off.release(); mate.release(); words.release(); word_base.release(); }
};

// the `[sbx] sort:` line of SBX_TIMING; by: what a name order puts in front ("" otherwise); the four wall-clock phases in ms
void print_sort_line(const sbx_sort_stats& st, const char* by, double open_ms, double read_ms, double sort_ms, double write_ms) {
    fprintf(stderr, "[sbx] sort: %sn_records_in=%llu n_records_out=%llu inflated_bytes=%llu sorted_stream_bytes=%llu compressed_bytes=%llu "
                    "key_bits=%u n_sort_passes=%u n_batches=%u ms_inflate=%.2f ms_index=%.2f ms_keys=%.2f ms_sort=%.2f ms_gather=%.2f "
                    "ms_deflate=%.2f ms_total_wall=%.1f (open %.1f, read pass %.1f, sort %.1f, write %.1f)\n", by,
            (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_out, (unsigned long long)st.inflated_bytes,
            (unsigned long long)st.sorted_stream_bytes, (unsigned long long)st.compressed_bytes, st.key_bits, st.n_sort_passes, st.n_batches,
            st.ms_inflate, st.ms_index, st.ms_keys, st.ms_sort, st.ms_gather, st.ms_deflate, st.ms_total_wall, open_ms, read_ms, sort_ms, write_ms);
}

// SBX_SORT_WINDOW_BYTES (tests, measurements): forces the windowed path with windows of this many bytes, rounded up to whole pieces.
// 0: unset (or not a positive decimal number).
uint64_t window_bytes_hook() { return env_u64("SBX_SORT_WINDOW_BYTES").value_or(0); }

constexpr uint64_t kWindowedPerRecord = 36;     // bytes per record while the keys are sorted: key, key2, len, val, val2, dest / out_off

// The read pass of both paths: the keys, lengths and -- with a store -- offsets of the records that take part while the batches arrive,
// and the one batch step around K9a.
struct KeyPass {
    sbx_ctx* c;
    bool use_filter;
    hipStream_t s;
    PassBooks<kSortAccWords> books;
    DevBuf<uint64_t> d_key, d_off, d_group_base;
    DevBuf<uint32_t> d_len, d_group_count;
    EventTimer t_k;
    double ms_keys = 0;
    uint64_t n_kept = 0;            // records that received a key in the batches so far
    uint64_t cur;                   // inflated offset of the file behind the batches so far

    KeyPass(sbx_ctx* c_, bool use_filter_, uint64_t u_first, hipStream_t s_) : c(c_), use_filter(use_filter_), s(s_), cur(u_first) {
        books.acc[kSortAccAnd] = ~0ull;
        books.init(s);
    }
    // K9a over a batch of for_each_record_batch; returns how many of its records received a key (they are [n_kept - that, n_kept)).
    // d_store: the resident record store -- the batch's bytes are copied behind those of the batches before, inside the timed
    // interval, and off[] is written -- or null: nothing is copied and no offset kept (the windowed path).
    uint64_t step(uint64_t nrec, uint64_t base, uint64_t next, uint8_t* d_store, uint64_t u_first) {
        const int32_t n_ref = (int32_t)c->hdr.refs.size();
        const size_t want = (size_t)(n_kept + nrec + 2);
        grow_keeping(d_key, (size_t)n_kept, want, s);
        if (d_store) grow_keeping(d_off, (size_t)n_kept, want, s);
        grow_keeping(d_len, (size_t)n_kept, want, s);
        if (use_filter) { d_group_count.ensure(sort_keys_groups(nrec) + 4); d_group_base.ensure(sort_keys_groups(nrec) + 4); }
        SortKeysArgs a{};
        a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.u_end = next - base;
        a.n_ref = n_ref; a.key_n_ref = n_ref; a.use_filter = use_filter ? 1u : 0u;
        a.store_delta = d_store ? (int64_t)base - (int64_t)u_first : 0;
        a.out_base = n_kept;
        a.key = d_key.p; a.off = d_store ? d_off.p : nullptr; a.len = d_len.p; a.acc = books.d_acc.p;
        t_k.start(s);
        if (d_store) copy_batch_to_store(c, d_store, u_first, cur, base, next, s);
        launch_sort_keys(a, d_group_count.p, d_group_base.p, s);
        t_k.stop(s);
        // (the next batch's K1 / K2 overwrite U and the descriptors: K9a and the copy end first)
        books.read_back(c, nrec, s);
        ms_keys += t_k.ms();
        const uint64_t kept = books.acc[kSortAccKept] - n_kept;
        n_kept = books.acc[kSortAccKept];
        cur = next;
        return kept;
    }
    bool bad() const { return books.acc[kSortAccBad] != 0; }
    // after the pass
    void refuse_bad() const {
        if (bad()) throw Error(SBX_EFORMAT, malformed_records_message(books.acc[kSortAccBad]));
    }
    void check_counts() const {
        if (!use_filter && n_kept != books.n)
            throw Error(SBX_EFORMAT, "internal error: " + std::to_string(n_kept) + " of " + std::to_string(books.n) + " records received a key");
        books.refuse_too_many(n_kept);
    }
    void times(sbx_sort_stats* st) const { st->ms_inflate = books.ms_inflate; st->ms_index = books.ms_index; st->ms_keys += ms_keys; }
};

// The coordinate sort of a file whose records do not stay on the device (or SBX_SORT_WINDOW_BYTES): the keys of the whole file are
// sorted as in sort_file, the order becomes one destination per record (K9d-1), and the sorted stream is written window by window
// (write_windows): the batches of the key pass whose destinations meet the window (K9d-2) are run again and K9d-3 puts their records
// in place.  The stream is cut into BGZF blocks exactly as write_permuted_bam cuts it, so the file is the resident path's byte for byte.
void sort_file_windowed(Standalone& c, OutputGuard& out_file, const std::vector<uint8_t>& header, bool use_filter, int level, uint64_t hook,
                        double w0, sbx_sort_stats* stats) {
    const uint64_t hlen = header.size();
    WindowBudget budget(c.get(), hlen, sortc::kSortWindowWords, hook);
    budget.fit(budget.est_records * kWindowedPerRecord, "the keys of its records, one read batch, the encoder and a window of one piece");
    hipStream_t s = c->stream.get();
    KeyPass keys(c.get(), use_filter, budget.u_first, s);
    DevBuf<uint32_t> d_rank;
    const unsigned long long* acc = keys.books.acc;
    const double w1 = wall_now();

    // ---- the key pass: K9a, nothing copied; the batches are saved ----
    sbx_sort_stats st{};
    std::vector<SavedBatch> saved;
    uint32_t n_batches = 0;
    for_each_record_batch(c.get(), budget.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
        saved.back().first_kept = keys.n_kept;
        saved.back().n_kept = keys.step(nrec, base, next, nullptr, 0);
        return !keys.bad();
    }, &saved);
    keys.refuse_bad();
    keys.check_counts();
    keys.times(&st);
    const uint64_t n_in = keys.books.n;
    const uint64_t n = keys.n_kept;
    const double w2 = wall_now();

    // ---- K9b, the offsets, K9d-1 and K9d-2 ----
    double ms_dest = 0;
    DevBuf<uint64_t> d_dest((size_t)n + 2);
    const std::vector<WindowSource> sources = one_open_source(c.get(), saved, n);
    BatchSpans spans;
    uint64_t total = hlen;
    {
        ResidentOrder order;
        sort_resident(keys.d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
        st.ms_sort = order.ms_sort;
        st.key_bits = order.key_bits; st.n_sort_passes = order.n_passes;
        const OutputPlan plan = plan_output(keys.d_len.p, order.perm, n, hlen, order.key2.p, s, &st.ms_gather);
        total = plan.total;
        if (total != hlen + acc[kSortAccBytes]) throw Error(SBX_EFORMAT, "internal error: the offsets of the sorted records do not add up");
        spans.upload(sources, n, s);
        EventTimer t;
        t.start(s);
        launch_window_dest(order.perm, order.key2.p, n, d_dest.p, s);
        spans.launch(d_dest.p, keys.d_len.p, s);
        t.stop(s);
        spans.read_back(s);
        ms_dest = t.ms();
        // keys, key2, val / val2 and the offsets go before the first window comes (order: end of this scope)
        keys.d_key.release();
    }

    // ---- the windows: K9d-3 for every saved batch that meets one ----
    const WindowedOutput w = write_windows(sources, s, out_file, header, total, budget, spans, level, [&](size_t, sbx_ctx*, const SavedBatch& sb,
                                           const RecordBatch& rb, const sortc::Window& win, uint8_t* d_win, unsigned long long* d_wacc, hipStream_t ws) {
        if (use_filter) {
            keys.d_group_count.ensure(sort_keys_groups(rb.nrec) + 4);
            keys.d_group_base.ensure(sort_keys_groups(rb.nrec) + 4);
            d_rank.ensure((size_t)rb.nrec + 2);
        }
        WindowScatterArgs a{};
        a.U = c->U(); a.desc = c->d_desc.p; a.n = rb.nrec; a.u_end = rb.next - rb.base; a.use_filter = use_filter ? 1u : 0u;
        a.first_kept = sb.first_kept; a.n_kept = sb.n_kept;
        a.dest = d_dest.p; a.len = keys.d_len.p; a.w0 = win.w0; a.w1 = win.w1; a.window = d_win; a.acc = d_wacc;
        launch_window_scatter(a, keys.d_group_count.p, keys.d_group_base.p, d_rank.p, ws);
    });
    out_file.disarm();
    const double w3 = w.w_planned, w4 = w.w_written;

    st.ms_gather += ms_dest + w.ms_scatter;
    st.n_records_in = n_in; st.n_records_out = n;
    st.inflated_bytes = budget.u_total; st.sorted_stream_bytes = total; st.compressed_bytes = w.compressed_bytes;
    st.n_batches = n_batches; st.n_windows = w.n_windows;
    st.ms_deflate = w.ms_deflate;
    st.ms_total_wall = (w4 - w0) * 1e3;
    if (getenv("SBX_TIMING")) {
        fprintf(stderr, "[sbx] sort-windows: n_windows=%u window_bytes=%llu n_batch_runs=%llu n_batches_skipped=%llu ms_dest=%.2f ms_scatter=%.2f "
                        "ms_inflate_replay=%.2f ms_index_replay=%.2f\n", st.n_windows, (unsigned long long)w.span, (unsigned long long)w.n_batch_runs,
                (unsigned long long)w.n_batches_skipped, ms_dest, w.ms_scatter, w.ms_inflate_replay, w.ms_index_replay);
        print_sort_line(st, "", (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
    }
    if (stats) *stats = st;
}

// order: 0 coordinate (sbx_sort_bam), nsc::kOrderLex, nsc::kOrderNatural (sbx_sort_bam_by_name)
void sort_file(const char* in_path, const char* out_path, const sbx_filter* filter, int level, uint32_t name_order, bool match_mates,
               int device, sbx_sort_stats* stats) {
    check_level(level);
    check_filter(filter);
    refuse_overwrite(in_path, out_path);
    const double w0 = wall_now();
    const bool use_filter = has_ops(filter);
    Standalone c = open_record_pass(in_path, device, filter, use_filter);
    OutputGuard out_file(out_path);
    std::string text, why;
    if (!sortc::sort_header_text(c->hdr.text.data(), c->hdr.text.size(), &text, &why, name_order ? "queryname" : "coordinate"))
        throw Error(SBX_EFORMAT, "SAM header: " + why);
    const std::vector<uint8_t> header = bam_header_bytes(text, c->hdr.refs);
    const uint64_t hlen = header.size();

    // per record: key, offset, length and K9b's second key and two values; a name order adds the key's offset, the -M word and
    // -- an estimate, the key store grows with the batches -- four key words
    // The coordinate order goes through windows when the records do not fit (or the hook says so); the name orders stay resident:
    // they plan without the "try", and the refusal of the plan is their answer.
    const uint64_t hook = name_order ? 0 : window_bytes_hook();
    std::optional<StorePlan> fits;
    if (name_order) fits = plan_record_store(c.get(), hlen, 48 + 16 + 32, "sorting");
    else if (!hook) fits = try_plan_record_store(c.get(), hlen, 48, "sorting");
    if (!fits) {
        sort_file_windowed(c, out_file, header, use_filter, level, hook, w0, stats);
        return;
    }
    const StorePlan& plan = *fits;
    const uint64_t u_total = plan.u_total, u_first = plan.u_first;
    hipStream_t s = c->stream.get();
    DevBuf<uint8_t> d_store((size_t)plan.store_bytes + 64);
    KeyPass keys(c.get(), use_filter, u_first, s);
    const unsigned long long* acc = keys.books.acc;
    NameKeys names;
    if (name_order) names.init(name_order, match_mates, s);
    const double w1 = wall_now();

    // ---- the read pass ----
    sbx_sort_stats st{};
    uint32_t n_batches = 0;
    bool names_ok = true;
    for_each_record_batch(c.get(), plan.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
        const uint64_t kept = keys.step(nrec, base, next, d_store.p, u_first);
        if (keys.bad()) return false;
        // K14a: the keys of the names of the records K9a kept, read from the store
        if (name_order) names_ok = names.add_batch(d_store.p, keys.d_off.p, keys.d_len.p, keys.n_kept - kept, kept, s, &st.ms_keys);
        return names_ok;
    });
    keys.refuse_bad();
    if (name_order) names.refuse_bad();
    keys.check_counts();
    keys.times(&st);
    const uint64_t n_in = keys.books.n, n = keys.n_kept;
    c.reset();                                       // the batch buffers make room for the sort and the output pieces
    const double w2 = wall_now();

    // ---- K9b (a name order: K14b + K9b, word by word) ----
    Stream stream;
    stream.create();
    s = stream.get();
    ResidentOrder order;
    if (name_order) {
        names.sort(keys.d_key.p, n, s, &order);
        SBX_HIP(hipStreamSynchronize(s));
        names.release();                             // the key store goes before the output pieces come
        order.hist.release();
        order.hist_base.release();
    } else {
        sort_resident(keys.d_key.p, n, acc[kSortAccOr] ^ acc[kSortAccAnd], s, &order);
    }
    // the keys are done with: one of their buffers holds the output offsets
    keys.d_key.release();
    st.ms_sort = order.ms_sort;

    // ---- offsets, K9c + deflate, piece by piece ----
    const WrittenBam w = write_store_output(out_file, header, d_store.p, keys.d_off.p, keys.d_len, order.perm, n, order.key2.p, level,
                                            &acc[kSortAccBytes], "sorted records", s, &st.ms_gather);
    out_file.disarm();
    const double w3 = w.w_planned, w4 = wall_now();
    st.n_records_in = n_in; st.n_records_out = n;
    st.inflated_bytes = u_total; st.sorted_stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
    st.key_bits = order.key_bits; st.n_sort_passes = order.n_passes; st.n_batches = n_batches;
    st.ms_deflate = w.ms_deflate;
    st.ms_total_wall = (w4 - w0) * 1e3;
    if (getenv("SBX_TIMING")) {
        char by[64] = "";
        if (name_order)
            snprintf(by, sizeof by, "order=%s%s words_sorted=%u ", name_order == nsc::kOrderNatural ? "natural" : "queryname",
                     match_mates ? "+mates" : "", names.words_sorted);
        print_sort_line(st, by, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
    }
    if (stats) *stats = st;
}

}  // namespace

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
        sort_file(in_path, out_path, filter, level, 0, false, device, stats);
    });
    // (the index is a pass of its own and not part of the sort's figures)
    return rc != SBX_OK ? rc : index_written_bam(out_path, with_index, device, err, errlen);
}

int sbx_sort_bam_by_name(const char* in_path, const char* out_path, const sbx_filter* filter, int level, int order, int match_mates,
                         int device, sbx_sort_stats* stats, char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        if (order != (int)nsc::kOrderLex && order != (int)nsc::kOrderNatural) throw Error(SBX_EINVAL, "order must be 1 (lexicographic) or 2 (natural)");
        sort_file(in_path, out_path, filter, level, (uint32_t)order, match_mates != 0, device, stats);
    });
}

}  // extern "C"
