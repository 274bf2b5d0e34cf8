// engine_markdup.cpp -- sbx_markdup: `sambamba markdup` (sambamba/markdup.d) on the device.
//
// Both paths below share their steps: EndsPass::step is the one batch step around K10a, pair_and_mark runs K10b and K10c with the
// pairing kernel as its one varying part, fill_counts fills the counters of the stats.  What a path adds is its own: where the
// records stay, and the output tail.
//
// The read pass is that of sbx_sort_bam (engine_store.hpp: every batch of records is copied into the resident record store); per
// batch K10a (markdup.hip) describes every record -- class, position key, score, name + RG hash.  Then, over the whole file: the
// pairable records are sorted by hash and paired inside the runs (K10b); the pairs are sorted by their three key words, the single
// ends and one marker per pair end by their two (K10c: LSD over the words with K9b's passes, a key gather between the words, digits
// that do not vary skipped); "not the first of its group" marks the duplicates; K10d patches the flags in the store; the file is
// written in input order -- with -r without the marked records -- by the writer sort uses.
//
// A file whose records do not fit the device next to one batch of the read pass takes the STREAMED path (markdup_streamed; also
// forced by SBX_MARKDUP_WINDOW_BYTES): no record store.  The key pass runs K10a and, next to it, K10e, which keeps the flag of every
// record and -- for the pairable ones -- the bytes K10b compares in a compact key store; the batches are saved.  K10b runs over the
// key store, K10c as ever.  The output stream is the input stream with some flag bytes changed and, with -r, some records left out:
// one kernel turns flag + duplicate bit into the length every record has in the output, a scan into its destination, and the stream
// is written window by window -- the saved batches whose records have a byte in the window are run again (run_record_batch) and K10f
// puts their records in place with byte 19 patched.  Batches and windows are both consecutive stretches of one ordered stream, so a
// batch is run again for at most the windows its stretch touches: the file goes through K1 + K2 about twice in all.  The file
// written is the resident path's byte for byte.  The budget of device memory, the spans of the batches, the choice of the window and
// the loop over windows and batches are engine_windows.hpp, shared with the windowed sort; what is here is the key pass, the marking,
// the output plan and the callback that launches K10f.
#include "engine_windows.hpp"
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

// the buffers of K10c that live to its end; the caller frees them when its timer has stopped (a free waits for the device)
struct GroupBuffers {
    DevBuf<uint32_t> d_first;
    DevBuf<uint64_t> d_w0, d_end2;
};

// K10c, shared by both paths: the pairs K10b made and the single ends, each sorted by their key words; d_dup[record] = 1 for every
// record that is not the first of its group.  Ends with the stream idle.
void mark_groups(const MdRecords& r, uint64_t n, uint64_t n_pairable, const uint32_t* d_mate, uint32_t ref_bits, WordSorter& sorter,
                 DevBuf<uint32_t>& d_cnt, DevBuf<uint64_t>& d_base, unsigned long long* d_acc, uint8_t* d_dup, hipStream_t s, GroupBuffers& g,
                 uint64_t* n_pairs_out, uint64_t* n_single_out) {
    DevBuf<uint32_t>& d_first = g.d_first;
    DevBuf<uint64_t>&d_w0 = g.d_w0, &d_end2 = g.d_end2;
    d_first.alloc((size_t)n_pairable / 2 + 2);
    const uint64_t n_pairs = compact(kMdPredPairFirst, r.cls, d_mate, n, d_cnt, d_base, d_first.p, s);
    d_w0.alloc((size_t)n_pairs + 2);
    DevBuf<uint64_t> d_w1((size_t)n_pairs + 2), d_w2((size_t)n_pairs + 2);
    d_end2.alloc((size_t)n_pairs + 2);
    launch_md_pair_keys(d_first.p, d_mate, n_pairs, r, ref_bits, d_w0.p, d_w1.p, d_w2.p, d_end2.p, s);
    launch_iota(sorter.idx(), n_pairs, s);
    sorter.sort_by(d_w2.p, n_pairs, d_acc, s);
    sorter.sort_by(d_w1.p, n_pairs, d_acc, s);
    sorter.sort_by(d_w0.p, n_pairs, d_acc, s);
    launch_md_pair_dups(sorter.idx(), d_w0.p, d_w1.p, n_pairs, d_first.p, d_mate, d_dup, s);
    d_w1.release(); d_w2.release();
    DevBuf<uint32_t> d_single((size_t)(n - 2 * n_pairs) + 2);
    const uint64_t n_single = compact(kMdPredSingle, r.cls, d_mate, n, d_cnt, d_base, d_single.p, s);
    const uint64_t m = 2 * n_pairs + n_single;
    DevBuf<uint64_t> d_v0((size_t)m + 2), d_v1((size_t)m + 2);
    DevBuf<uint32_t> d_rec((size_t)m + 2);
    launch_md_single_entries(d_w0.p, d_end2.p, n_pairs, d_single.p, n_single, r, d_v0.p, d_v1.p, d_rec.p, d_acc, s);
    launch_iota(sorter.idx(), m, s);
    sorter.sort_by(d_v1.p, m, d_acc, s);
    sorter.sort_by(d_v0.p, m, d_acc, s);
    launch_md_single_dups(sorter.idx(), d_v0.p, d_v1.p, d_rec.p, m, d_dup, s);
    SBX_HIP(hipStreamSynchronize(s));
    *n_pairs_out = n_pairs;
    *n_single_out = n_single;
}

// what both paths know before the first batch: the output header, the libraries of the read groups (on the device), the key widths
struct MdJob {
    std::vector<uint8_t> header;
    int32_t n_ref = 0;
    uint32_t ref_bits = 0;
    uint64_t hash_mask = ~0ull;
    std::string rg_ids;
    std::vector<uint32_t> rg_off;
    std::vector<int32_t> library_of;
    DevBuf<char> d_rg_ids;
    DevBuf<uint32_t> d_rg_off;
    DevBuf<int32_t> d_rg_lib;
    void upload(hipStream_t s) {
        d_rg_ids.alloc(rg_ids.size() + 1);
        d_rg_off.alloc(rg_off.size() + 1);
        d_rg_lib.alloc(library_of.size() + 1);
        if (rg_off.empty()) return;
        SBX_HIP(hipMemcpyAsync(d_rg_ids.p, rg_ids.data(), rg_ids.size(), hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(d_rg_off.p, rg_off.data(), rg_off.size() * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(d_rg_lib.p, library_of.data(), library_of.size() * 4, hipMemcpyHostToDevice, s));
    }
    LibTable table() const { return LibTable{d_rg_ids.p, d_rg_off.p, d_rg_lib.p, (int32_t)rg_off.size()}; }
};

// the `[sbx] markdup:` line of SBX_TIMING; the four wall-clock phases in ms
void print_markdup_line(const sbx_markdup_stats& st, double open_ms, double read_ms, double dup_ms, double write_ms) {
    fprintf(stderr, "[sbx] markdup: n_records_in=%llu n_records_out=%llu n_end_pairs=%llu n_single_ends=%llu n_unmatched_pairs=%llu "
                    "n_duplicates=%llu inflated_bytes=%llu stream_bytes=%llu compressed_bytes=%llu n_sort_passes=%u n_batches=%u "
                    "ms_inflate=%.2f ms_index=%.2f ms_ends=%.2f ms_pairing=%.2f ms_groups=%.2f ms_gather=%.2f ms_deflate=%.2f "
                    "ms_total_wall=%.1f (open %.1f, read pass %.1f, duplicates %.1f, write %.1f)\n",
            (unsigned long long)st.n_records_in, (unsigned long long)st.n_records_out, (unsigned long long)st.n_end_pairs,
            (unsigned long long)st.n_single_ends, (unsigned long long)st.n_unmatched_pairs, (unsigned long long)st.n_duplicates,
            (unsigned long long)st.inflated_bytes, (unsigned long long)st.stream_bytes, (unsigned long long)st.compressed_bytes,
            st.n_sort_passes, st.n_batches, st.ms_inflate, st.ms_index, st.ms_ends, st.ms_pairing, st.ms_groups, st.ms_gather, st.ms_deflate,
            st.ms_total_wall, open_ms, read_ms, dup_ms, write_ms);
}

// SBX_MARKDUP_WINDOW_BYTES (tests, measurements): forces the streamed path with windows of this many bytes, rounded up to whole
// pieces.  0: unset (or not a positive decimal number).
uint64_t markdup_window_hook() { return env_u64("SBX_MARKDUP_WINDOW_BYTES").value_or(0); }

// Bytes of per-record arrays at the peak of the streamed path, which is K10c.  The key pass keeps 39 per record (off 8, len 4, class 1,
// position key 8, score 4, hash 8, rg_at 4, flag 2); pairing adds mate 4, dup 1 and the hash sort's two (key, index) buffers, 24 per
// pairable record; for K10c the hashes (8) and the key store are gone and the pair words (4 x 8 per pair = 16 per paired record), the
// first-of-pair list (2) and the single-end entries (20 per entry, at most one per record) come: 39 - 8 + 5 + 24 + 2 + 16 + 20 = 98.
// While the windows are written 17 remain (len 4, output length 4, destination 8, flag byte 1).
constexpr uint64_t kStreamedPerRecord = 98;
// Estimate of the key store per record of the file: an entry is 2 + l_read_name + the RG value's length, only pairable records have
// one, and the store grows by half whenever a batch does not fit (the old and the new buffer exist side by side for that moment).
constexpr uint64_t kStreamedKeyBytes = 48;

// The read pass of both paths: the per-record arrays K10a fills while the batches arrive, and the one batch step around it.
struct EndsPass {
    sbx_ctx* c;
    const MdJob& job;
    hipStream_t s;
    PassBooks<kMdAccWords> books;
    DevBuf<uint64_t> d_off, d_pos_key, d_hash;
    DevBuf<uint32_t> d_len, d_score, d_rg_at;
    DevBuf<uint8_t> d_cls;
    EventTimer t_k;
    double ms_ends = 0;
    uint64_t cur;                   // inflated offset of the file behind the batches so far

    EndsPass(sbx_ctx* c_, const MdJob& job_, uint64_t u_first, hipStream_t s_) : c(c_), job(job_), s(s_), cur(u_first) { books.init(s); }
    MdRecords records() const { return MdRecords{d_off.p, d_len.p, d_cls.p, d_pos_key.p, d_score.p, d_hash.p, d_rg_at.p}; }
    // K10a over a batch of for_each_record_batch (books.admit(nrec) has said yes).  d_store: the resident record store -- the batch's
    // bytes are copied behind those of the batches before, inside the timed interval, and off[] holds store offsets -- or null
    // (the streamed path: K10e overwrites off[] of the pairable records).  behind(): what the path queues behind K10a and in front
    // of the read-back that ends the step.
    template <class Behind>
    void step(uint64_t nrec, uint64_t base, uint64_t next, uint8_t* d_store, uint64_t u_first, Behind&& behind) {
        const uint64_t n = books.n;
        const size_t want = (size_t)(n + nrec + 2);
        grow_keeping(d_off, (size_t)n, want, s);
        grow_keeping(d_pos_key, (size_t)n, want, s);
        grow_keeping(d_hash, (size_t)n, want, s);
        grow_keeping(d_len, (size_t)n, want, s);
        grow_keeping(d_score, (size_t)n, want, s);
        grow_keeping(d_rg_at, (size_t)n, want, s);
        grow_keeping(d_cls, (size_t)n, want, s);
        MdEndsArgs a{};
        a.U = c->U(); a.desc = c->d_desc.p; a.n = nrec; a.u_end = next - base;
        a.n_ref = job.n_ref; a.ref_bits = job.ref_bits; a.hash_mask = job.hash_mask;
        a.store_delta = d_store ? (int64_t)base - (int64_t)u_first : 0;
        a.out_base = n;
        a.lib = job.table();
        a.r = records();
        a.acc = books.d_acc.p;
        t_k.start(s);
        if (d_store) copy_batch_to_store(c, d_store, u_first, cur, base, next, s);
        launch_md_ends(a, s);
        t_k.stop(s);
        behind();
        // (the next batch's K1 / K2 overwrite U and the descriptors: K10a and the copy end first)
        books.read_back(c, nrec, s);
        ms_ends += t_k.ms();
        cur = next;
    }
    bool bad() const { return books.acc[kMdAccBad] != 0; }
    // after the pass
    void refuse() const {
        books.refuse_too_many();
        if (bad()) throw Error(SBX_EFORMAT, malformed_records_message(books.acc[kMdAccBad]));
    }
};

// the buffers of K10b and K10c (the caller lets go of them: when, sets the peak of its path), and what the two count
struct MarkWork {
    DevBuf<uint32_t> d_mate, d_cnt;
    DevBuf<uint64_t> d_base;
    WordSorter sorter;
    GroupBuffers groups;
    explicit MarkWork(uint64_t n) : d_mate((size_t)n + 2), d_cnt(md_groups(n) + 4), d_base(md_groups(n) + 4) {}
};
struct MarkCounts { uint64_t n_pairable = 0, n_pairs = 0, n_single = 0; };

// K10b, then K10c, over the n records of the pass: d_dup[record] = 1 for every duplicate.  What varies between the paths:
// pair_runs(sorted hashes, their records, n_pairable, d_mate) is the pairing kernel -- it compares names in the record store or in
// the key store --; between() lets go of what the path needs no more once the pairs are made; behind() queues what the path counts
// into ms_groups behind K10c.  Ends with the accumulators read back and the stream idle; ms_pairing, ms_groups and n_sort_passes of
// *st are set.
template <class PairRuns, class Between, class Behind>
MarkCounts pair_and_mark(const MdRecords& r, uint64_t n, uint32_t ref_bits, MarkWork& w, PassBooks<kMdAccWords>& books, uint8_t* d_dup, hipStream_t s,
                   sbx_markdup_stats* st, PairRuns&& pair_runs, Between&& between, Behind&& behind) {
    MarkCounts k;
    EventTimer t_pair, t_groups;
    t_pair.start(s);
    launch_fill32(w.d_mate.p, kMdNone, n, s);
    SBX_HIP(hipMemsetAsync(d_dup, 0, (size_t)n + 2, s));
    k.n_pairable = compact(kMdPredPairable, r.cls, w.d_mate.p, n, w.d_cnt, w.d_base, w.sorter.idx(), s);
    w.sorter.sort_by(r.hash, k.n_pairable, books.d_acc.p, s);
    pair_runs(w.sorter.keys(), w.sorter.idx(), k.n_pairable, w.d_mate.p);
    t_pair.stop(s);
    SBX_HIP(hipStreamSynchronize(s));
    st->ms_pairing = t_pair.ms();
    between();
    t_groups.start(s);
    mark_groups(r, n, k.n_pairable, w.d_mate.p, ref_bits, w.sorter, w.d_cnt, w.d_base, books.d_acc.p, d_dup, s, w.groups, &k.n_pairs, &k.n_single);
    behind();
    t_groups.stop(s);
    SBX_HIP(hipMemcpyAsync(books.acc, books.d_acc.p, sizeof books.acc, hipMemcpyDeviceToHost, s));
    SBX_HIP(hipStreamSynchronize(s));
    st->ms_groups = t_groups.ms();
    st->n_sort_passes = w.sorter.passes;
    return k;
}

// the counters of the stats, and the times of the read pass (books.acc: as read back behind the last kernel that counts)
void fill_counts(const EndsPass& pass, const MarkCounts& k, uint64_t n_out, uint32_t n_batches, sbx_markdup_stats* st) {
    const unsigned long long* acc = pass.books.acc;
    st->n_records_in = pass.books.n; st->n_records_out = n_out;
    st->n_end_pairs = k.n_pairs; st->n_single_ends = k.n_single; st->n_unmatched_pairs = acc[kMdAccUnmatched]; st->n_duplicates = acc[kMdAccDup];
    st->n_batches = n_batches;
    st->ms_inflate = pass.books.ms_inflate; st->ms_index = pass.books.ms_index; st->ms_ends = pass.ms_ends;
}

// The streamed path (see the head of this file).  hook: SBX_MARKDUP_WINDOW_BYTES or 0.
void markdup_streamed(Standalone& c, OutputGuard& out_file, MdJob& job, bool remove, int level, uint64_t hook, double w0,
                      sbx_markdup_stats* stats, sbx_markdup_stream_stats* stream_stats) {
    const std::vector<uint8_t>& header = job.header;
    const uint64_t hlen = header.size();
    WindowBudget budget(c.get(), hlen, sortc::kMarkdupWindowWords, hook);
    const uint64_t arrays_est = budget.est_records * kStreamedPerRecord, keys_est = budget.est_records * kStreamedKeyBytes;
    budget.fit(arrays_est + keys_est,
               std::to_string(arrays_est) + " for the per-record arrays, " + std::to_string(keys_est) + " for the key store (an estimate), " +
                   std::to_string(WindowBudget::kMinBatch) + " for one read batch, " + std::to_string(budget.out_reserve) +
                   " for the encoder and " + std::to_string(budget.cap_bytes) + " for a window of one piece");
    hipStream_t s = c->stream.get();
    job.upload(s);
    EndsPass pass(c.get(), job, budget.u_first, s);
    DevBuf<uint64_t> d_key_off, d_tile_sum;
    DevBuf<uint32_t> d_key_len;
    DevBuf<uint8_t> d_keys;
    DevBuf<uint16_t> d_flag;
    unsigned long long* acc = pass.books.acc;
    const double w1 = wall_now();

    // ---- the key pass: K10a + K10e, nothing copied; the batches are saved ----
    sbx_markdup_stats st{};
    sbx_markdup_stream_stats ss{};
    EventTimer t_m, t_e;
    std::vector<SavedBatch> saved;
    uint64_t key_bytes = 0;
    uint32_t n_batches = 0;
    for_each_record_batch(c.get(), budget.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
        if (!pass.books.admit(nrec)) return false;
        const uint64_t first = pass.books.n;
        grow_keeping(d_flag, (size_t)first, (size_t)(first + nrec + 2), s);
        d_key_len.ensure((size_t)nrec + 2);
        d_key_off.ensure((size_t)nrec + 2);
        d_tile_sum.ensure(len_tiles(nrec) + 2);
        MdKeyArgs k{};
        k.U = c->U(); k.desc = c->d_desc.p; k.n = nrec; k.out_base = first;
        k.flag = d_flag.p; k.key_len = d_key_len.p; k.key_off = d_key_off.p;
        uint64_t key_end = key_bytes;
        pass.step(nrec, base, next, nullptr, 0, [&] {
            k.r = pass.records();
            t_m.start(s);
            launch_md_key_measure(k, s);
            launch_sorted_offsets(d_key_len.p, nullptr, nrec, key_bytes, d_tile_sum.p, d_key_off.p, s);
            t_m.stop(s);
            if (nrec) SBX_HIP(hipMemcpyAsync(&key_end, d_key_off.p + nrec, 8, hipMemcpyDeviceToHost, s));
        });
        ss.ms_keys += t_m.ms();
        saved.back().first_kept = first;
        saved.back().n_kept = nrec;
        if (pass.bad()) return false;
        grow_keeping(d_keys, (size_t)key_bytes, (size_t)key_end + 64, s);       // (SBX_ENOMEM when the keys do not fit)
        k.key_store = d_keys.p;
        t_e.start(s);
        launch_md_key_emit(k, s);
        t_e.stop(s);
        // (the next batch's K1 / K2 overwrite U and the descriptors: K10e ends first)
        SBX_HIP(hipStreamSynchronize(s));
        ss.ms_keys += t_e.ms();
        key_bytes = key_end;
        return true;
    }, &saved);
    pass.refuse();
    const uint64_t n = pass.books.n;
    const double w2 = wall_now();

    // ---- K10b over the key store, K10c ----
    const MdRecords r = pass.records();
    DevBuf<uint8_t> d_dup((size_t)n + 2);
    MarkCounts marked;
    {
        MarkWork w(n);
        w.sorter.reserve(n);
        marked = pair_and_mark(
            r, n, job.ref_bits, w, pass.books, d_dup.p, s, &st,
            [&](const uint64_t* hashes, const uint32_t* idx, uint64_t n_pairable, uint32_t* d_mate) {
                launch_md_pair_runs_keys(hashes, idx, n_pairable, d_keys.p, r, d_mate, s);
            },
            [&] { pass.d_hash.release(); d_keys.release(); pass.d_off.release(); pass.d_rg_at.release(); }, [] {});
    }
    pass.d_pos_key.release(); pass.d_score.release(); pass.d_cls.release();

    // ---- the output plan: lengths in the output, destinations, the span of every batch ----
    DevBuf<uint8_t> d_hi((size_t)n + 2);
    DevBuf<uint32_t> d_out_len((size_t)n + 2);
    DevBuf<uint64_t> d_dest((size_t)n + 2);
    const std::vector<WindowSource> sources = one_open_source(c.get(), saved, n);
    BatchSpans spans;
    uint64_t total = hlen;
    {
        spans.upload(sources, n, s);
        d_tile_sum.ensure(len_tiles(n) + 2);
        EventTimer t;
        t.start(s);
        launch_md_out_plan(d_flag.p, d_dup.p, pass.d_len.p, n, remove ? 1u : 0u, d_hi.p, d_out_len.p, pass.books.d_acc.p, s);
        launch_sorted_offsets(d_out_len.p, nullptr, n, hlen, d_tile_sum.p, d_dest.p, s);
        spans.launch(d_dest.p, d_out_len.p, s);
        t.stop(s);
        if (n) SBX_HIP(hipMemcpyAsync(&total, d_dest.p + n, 8, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(acc, pass.books.d_acc.p, sizeof pass.books.acc, hipMemcpyDeviceToHost, s));
        spans.read_back(s);
        ss.ms_plan = t.ms();
    }
    d_flag.release(); d_dup.release(); d_tile_sum.release(); d_key_len.release(); d_key_off.release();
    const uint64_t n_out = acc[kMdAccKept];
    if (!remove && (n_out != n || total != hlen + acc[kMdAccBytes])) throw Error(SBX_EFORMAT, "internal error: the offsets of the records do not add up");

    // ---- the windows: K10f for every saved batch that meets one ----
    const WindowedOutput w = write_windows(sources, s, out_file, header, total, budget, spans, level, [&](size_t, sbx_ctx*, const SavedBatch& sb,
                                           const RecordBatch& rb, const sortc::Window& win, uint8_t* d_win, unsigned long long* d_wacc, hipStream_t ws) {
        MdScatterArgs a{};
        a.U = c->U(); a.desc = c->d_desc.p; a.n = rb.nrec; a.u_end = rb.next - rb.base; a.first = sb.first_kept;
        a.dest = d_dest.p; a.len = pass.d_len.p; a.out_len = d_out_len.p; a.hi = d_hi.p;
        a.w0 = win.w0; a.w1 = win.w1; a.window = d_win; a.acc = d_wacc;
        launch_md_window_scatter(a, ws);
    });
    out_file.disarm();
    const double w3 = w.w_planned, w4 = w.w_written;

    ss.ms_scatter = w.ms_scatter; ss.ms_inflate_replay = w.ms_inflate_replay; ss.ms_index_replay = w.ms_index_replay;
    ss.n_windows = w.n_windows; ss.n_batch_runs = (uint32_t)w.n_batch_runs; ss.n_batches_skipped = (uint32_t)w.n_batches_skipped;
    st.ms_gather = ss.ms_plan + ss.ms_scatter;
    fill_counts(pass, marked, n_out, n_batches, &st);
    st.ms_ends += ss.ms_keys;                            // (K10e counts as part of the ends)
    st.inflated_bytes = budget.u_total; st.stream_bytes = total; st.compressed_bytes = w.compressed_bytes;
    st.ms_deflate = w.ms_deflate;
    st.ms_total_wall = (w4 - w0) * 1e3;
    ss.window_bytes = w.span; ss.key_store_bytes = key_bytes; ss.n_key_records = marked.n_pairable;
    if (getenv("SBX_TIMING")) {
        fprintf(stderr, "[sbx] markdup-stream: n_windows=%u window_bytes=%llu n_batch_runs=%u n_batches_skipped=%u key_store_bytes=%llu "
                        "n_key_records=%llu ms_keys=%.2f ms_plan=%.2f ms_scatter=%.2f ms_inflate_replay=%.2f ms_index_replay=%.2f\n",
                ss.n_windows, (unsigned long long)ss.window_bytes, ss.n_batch_runs, ss.n_batches_skipped, (unsigned long long)ss.key_store_bytes,
                (unsigned long long)ss.n_key_records, ss.ms_keys, ss.ms_plan, ss.ms_scatter, ss.ms_inflate_replay, ss.ms_index_replay);
        print_markdup_line(st, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
    }
    if (stats) *stats = st;
    if (stream_stats) {
        ss.struct_size = stream_stats->struct_size;
        memcpy(stream_stats, &ss, sizeof ss);
    }
}

}  // namespace

extern "C" {

int sbx_markdup_header_text(const char* text, size_t n, const char* pg_command_line, char* out, size_t cap, size_t* out_len) {
    if (!text && n) return SBX_EINVAL;
    std::string t;
    if (!mdc::markdup_header_text(text ? text : "", n, pg_command_line, &t, nullptr)) return SBX_EFORMAT;
    return copy_to_caller(t, out, cap, out_len);
}

int sbx_markdup_run(const char* in_path, const char* out_path, int remove_duplicates, int level, const char* pg_command_line, int device,
                    sbx_markdup_stats* stats, sbx_markdup_stream_stats* stream_stats, char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!in_path || !out_path) throw Error(SBX_EINVAL, "null argument");
        if (stream_stats) {
            if (stream_stats->struct_size < sizeof(sbx_markdup_stream_stats))
                throw Error(SBX_EINVAL, "sbx_markdup_stream_stats: struct_size " + std::to_string(stream_stats->struct_size) + " is smaller than the struct");
            const uint32_t size = stream_stats->struct_size;                 // the resident path: everything else is 0
            memset(stream_stats, 0, sizeof *stream_stats);
            stream_stats->struct_size = size;
        }
        check_level(level);
        refuse_overwrite(in_path, out_path);
        const double w0 = wall_now();
        Standalone c = open_record_pass(in_path, device, nullptr, false);
        OutputGuard out_file(out_path);
        MdJob job;
        const int32_t n_ref = job.n_ref = (int32_t)c->hdr.refs.size();
        std::string text, why;
        if (!mdc::markdup_header_text(c->hdr.text.data(), c->hdr.text.size(), pg_command_line, &text, &why)) throw Error(SBX_EFORMAT, "SAM header: " + why);
        job.header = bam_header_bytes(text, c->hdr.refs);
        const std::vector<uint8_t>& header = job.header;
        const uint64_t hlen = header.size();

        // read groups -> libraries
        sortc::ParsedHeader ph;
        sortc::parse_header(c->hdr.text.data(), c->hdr.text.size(), &ph, nullptr);
        const int32_t n_lib = mdc::read_group_libraries(ph, &job.library_of);
        if (!mdc::key_fits(n_lib, n_ref))
            throw Error(SBX_EUNSUPPORTED, std::to_string(n_lib) + " libraries and " + std::to_string(n_ref) + " references do not fit the 64-bit position key");
        job.ref_bits = mdc::ref_bits_of(n_ref);
        for (const sortc::HeaderLine& l : ph.rg) { job.rg_off.push_back((uint32_t)job.rg_ids.size()); job.rg_ids += l.id; job.rg_ids.push_back('\0'); }
        if (const char* e = getenv("SBX_MARKDUP_HASH_BITS")) {
            const unsigned long b = strtoul(e, nullptr, 10);
            if (b < 64) job.hash_mask = (1ull << b) - 1ull;
        }

        // The records stay on the device when they fit; otherwise (or when the hook says so) the file is streamed.
        const uint64_t hook = markdup_window_hook();
        const std::optional<StorePlan> fits = hook ? std::nullopt : try_plan_record_store(c.get(), hlen, 96, "marking the duplicates of");
        if (!fits) {
            markdup_streamed(c, out_file, job, remove_duplicates != 0, level, hook, w0, stats, stream_stats);
            return;
        }
        const StorePlan& plan = *fits;
        const uint64_t u_first = plan.u_first, u_total = plan.u_total;
        hipStream_t s = c->stream.get();
        DevBuf<uint8_t> d_store((size_t)plan.store_bytes + 64);
        job.upload(s);
        EndsPass pass(c.get(), job, u_first, s);
        const double w1 = wall_now();

        // ---- the read pass ----
        sbx_markdup_stats st{};
        uint32_t n_batches = 0;
        for_each_record_batch(c.get(), plan.batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
            if (!pass.books.admit(nrec)) return false;
            pass.step(nrec, base, next, d_store.p, u_first, [] {});
            return !pass.bad();
        });
        pass.refuse();
        const uint64_t n = pass.books.n;
        c.reset();                                       // the batch buffers make room for the sorts and the output pieces
        const double w2 = wall_now();

        // ---- K10b: pairing; K10c: pair groups, fragment groups; K10d ----
        Stream stream;
        stream.create();
        s = stream.get();
        const MdRecords r = pass.records();
        MarkWork work(n);
        DevBuf<uint8_t> d_dup((size_t)n + 2), d_keep((size_t)n + 2);
        work.sorter.reserve(n);
        DevBuf<uint32_t> d_perm;            // the records that are written, in file order
        uint64_t n_out = n;
        const MarkCounts marked = pair_and_mark(
            r, n, job.ref_bits, work, pass.books, d_dup.p, s, &st,
            [&](const uint64_t* hashes, const uint32_t* idx, uint64_t n_pairable, uint32_t* d_mate) {
                launch_md_pair_runs(hashes, idx, n_pairable, d_store.p, r, d_mate, s);
            },
            [&] { pass.d_hash.release(); },
            [&] {
                launch_md_patch_flags(d_store.p, r.off, d_dup.p, n, remove_duplicates ? 1u : 0u, d_keep.p, pass.books.d_acc.p, s);
                d_perm.alloc((size_t)n + 2);
                if (remove_duplicates) n_out = compact(kMdPredKeep, d_keep.p, nullptr, n, work.d_cnt, work.d_base, d_perm.p, s);
                else launch_iota(d_perm.p, n, s);
            });
        work.sorter = WordSorter();
        work.groups = GroupBuffers();
        work.d_mate.release(); d_dup.release(); d_keep.release();
        pass.d_pos_key.release(); pass.d_score.release(); pass.d_rg_at.release(); pass.d_cls.release();

        // ---- the output ----
        DevBuf<uint64_t> d_out_off((size_t)n_out + 2);
        const WrittenBam w = write_store_output(out_file, header, d_store.p, pass.d_off.p, pass.d_len, d_perm.p, n_out, d_out_off.p, level,
                                                remove_duplicates ? nullptr : &pass.books.acc[kMdAccBytes], "records", s, &st.ms_gather);
        out_file.disarm();
        const double w3 = w.w_planned, w4 = wall_now();
        fill_counts(pass, marked, n_out, n_batches, &st);
        st.inflated_bytes = u_total; st.stream_bytes = w.stream_bytes; st.compressed_bytes = w.compressed_bytes;
        st.ms_deflate = w.ms_deflate;
        st.ms_total_wall = (w4 - w0) * 1e3;
        if (getenv("SBX_TIMING")) print_markdup_line(st, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w4 - w3) * 1e3);
        if (stats) *stats = st;
    });
}

int sbx_markdup(const char* in_path, const char* out_path, int remove_duplicates, int level, const char* pg_command_line, int device,
                sbx_markdup_stats* stats, char* err, size_t errlen) {
    return sbx_markdup_run(in_path, out_path, remove_duplicates, level, pg_command_line, device, stats, nullptr, err, errlen);
}

}  // extern "C"
