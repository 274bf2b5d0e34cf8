// engine_ctx.hpp -- what the translation units of the engine (engine*.cpp) share: the context behind the C ABI (include/sbx_depth.h),
// the work list of a launch, the result words of a pass, and the few functions one unit needs of another.
//
// The unit of work is a WORK LIST of chain runs (kernels.hpp ChainRun): the whole file from its first record on,
// or -- with -L, with sbx_run_batch / sbx_run_interval -- the BGZF block runs that hold the merged BAI chunks of the
// requested regions (RandomAccessManager.getChunks / getReads, randomaccessmanager.d:247-348; StreamChunksSupplier,
// inputstream.d:257-345), every run starting at a record boundary the index names.  Only those blocks are uploaded
// and inflated; the inflated pieces are laid out back to back in one device buffer.
#pragma once
#include <atomic>
#include <mutex>

#include "common.hpp"
#include "entry_util.hpp"
#include "file_run.hpp"
#include "host_io.hpp"
#include "host_res.hpp"
#include "kernels.hpp"

namespace sbx {

// Padding behind the compressed bytes on the device.  The fast K1a lane (inflate2_core.hpp) prefetches its input 16 bytes at a time and
// tests the end of the block's payload only between deflate blocks: on a corrupt stream a lane may go on decoding what follows its
// block until its output position passes ISIZE.  Every literal/length symbol it consumes (<= 15 bits, <= 48 with a match) produces at
// least one output byte of at most 65536, and it reads at most kMaxSeg block headers (<= 600 bytes each), so it can run at most
// ~128 KiB beyond its own block -- into the following blocks, or, for the last blocks of a batch, into this padding.  (The general
// kernel, which re-decodes every block the fast one flags, tests its input per symbol.)
constexpr size_t kCompPad = 192 * 1024;

// The work list of a launch: file runs, and the per-block tables of the launch in compacted coordinates
// (block i of the launch is file block file_blk[i]; its payload sits at comp_off[i] of d_comp, its inflated
// bytes at out_off[i] of d_U).
struct WorkList {
    std::vector<FileRun> runs;
    std::vector<uint32_t> file_blk, comp_len, isize, run_of;
    std::vector<uint64_t> comp_off, out_off;        // out_off has n + 1 entries
    std::vector<ChainRun> chain;
    struct Range { uint64_t file_off, len, dst; };
    std::vector<Range> ranges;                      // file bytes -> d_comp (only when the file is not preloaded)
    uint64_t comp_bytes = 0, u_bytes = 0;
    size_t n_blocks() const { return file_blk.size(); }
};

// result words of a pass, written by async copies into pinned host memory and read after one synchronisation
struct HostResults {
    uint32_t flags[4];
    uint32_t n_active, n_deep;
    IndexStats st[kIndexStatSlots];
    uint64_t last_state;
    uint32_t max_partners, n_rewalked;
    unsigned long long tok_bytes[64];
    uint64_t straddler;           // open-ended run: start of the record that continues behind it (kOffUnknown: none)
};

// The words of sbx_ctx::d_flag.  K2 sees words 0 .. 2 as IndexArgs::flags[0 .. 2] and the straddler as flags + 8; every other word
// reaches its kernel as a pointer of its own.  The host reads them back into HostResults after a synchronisation.
//   kFlagFirstBad       the chain checks of index.hip: lowest block whose chain is inconsistent (atomicMin; 0xFFFFFFFF: none).
//                       index_pass reads it and sends the pass to repair_chain.
//   kFlagFailedInflate  index.hip: lowest block whose inflate status is not 0 (atomicMin; 0xFFFFFFFF: none).  index_pass reads it and throws.
//   kFlagDescOverflow   the record scans of index.hip: != 0, the descriptor array is too small (the describe kernel then writes nothing).
//                       index_pass reads it and repeats the pass with the exact capacity.
//   kFlagTicket         cleared and copied back with the three before it; no kernel takes it (the tickets of the scans live in d_scan_part).
//   kFlagRewalked       launch_rewalk_mismatched / launch_chain_repair add the blocks they walked again; repair_chain clears it before
//                       every launch and reads it after.
//   kFlagMaxPartners    launch_max_u32 over n_partners (-m); accumulate_pass reads it and chooses between pairs and partner lists;
//                       bit 31: one name in two samples next to a same-sample partner, which accumulate_pass refuses.
//   kFlagMatesOverflow  launch_accumulate_mates (-m, `base`): != 0, more overlapping same-name records on a position than K7 pairs;
//                       accumulate_pass reads it and refuses.
//   kFlagCrossFile      launch_cross_file_mates (-m, several BAMs): != 0, a same-name pair lies in two files; run_files clears and reads it.
//   kFlagStraddler      two words, 64 bits: the chain walk of an open-ended run leaves the start of the record that continues behind the
//                       run (atomicMin; kOffUnknown: none).  index_pass reads it in index mode, for for_each_record_batch.
enum FlagWord : uint32_t {
    kFlagFirstBad = 0, kFlagFailedInflate = 1, kFlagDescOverflow = 2, kFlagTicket = 3, kFlagRewalked = 4, kFlagMaxPartners = 5,
    kFlagMatesOverflow = 6, kFlagCrossFile = 7, kFlagStraddler = 8, kFlagWords = 12
};
static_assert(kFlagTicket + 1 == sizeof(HostResults::flags) / 4, "HostResults::flags mirrors the words up to the ticket");

}  // namespace sbx

using namespace sbx;

constexpr size_t kStageBytes = 32u << 20;   // one pinned staging buffer of the upload
constexpr int kStages = 4;                   // ... of a ring of four

struct sbx_ctx {
    std::string last_error;
    std::mutex err_mu;                       // last_error: sbx_prefetch_interval may run on a second thread
    std::atomic<double> upload_ms{0.0};      // wall clock of the last upload (make_resident)
    // several BAMs (MultiBamReader, multireader.d:244): this context is the first file and owns the merged view;
    // every further file is a complete single-file context of its own
    std::vector<sbx_ctx*> members;
    bool in_group = false;                   // this context is one file of several (the primary or a member): its tiles get merged
    // the last run kept ONE word per tile position and sample, {bases counted : 16 | depth : 16}, instead of the seven counters
    // (region / window modes without -m: launch_accumulate `compact`); sbx_depth_base_tile then knows `covered` only
    bool compact_counters = false;
    int device = 0;
    FileMap file;
    BlockTable blocks;
    BamHeaderInfo hdr;
    BaiIndex bai;
    bool has_index = false;

    // parameters
    int mode = SBX_MODE_BASE;
    uint32_t min_bq = 0;
    bool fix_mate = false, combined = false;
    uint32_t window = 0, overlap = 0;
    std::vector<uint32_t> thresholds;
    sbx_filter filter;
    std::vector<sbx_region> regions;
    bool index_mode = false;        // sbx_build_index: every record is described, no index / sort order / read group is required, no K3
    bool filter_every = false;      // sbx_sort_bam with a filter (index mode): K2 asks the filter about every record (IndexArgs::filter_every)
    // read ownership of the next run (sbx_run_interval_owned): own_ref >= 0
    int32_t own_ref = -1;
    uint32_t own_beg = 0, own_end = 0;

    // compressed input on the device: the whole file (sbx_preload) or the blocks of the current work list
    bool preloaded = false;
    DevBuf<uint8_t> d_comp;
    WorkList wl;                    // the work list whose tables (and, unless preloaded, payload bytes) are resident
    bool wl_resident = false;
    DevBuf<uint64_t> d_comp_off, d_out_off;
    DevBuf<uint32_t> d_comp_len, d_isize, d_run_of, d_status;
    DevBuf<ChainRun> d_runs;
    // sbx_stream_base_rows: two pieces of text in flight (device buffer, pinned host buffer, events)
    DevBuf<uint8_t> d_fmt_text2[2];
    PinnedBuf<uint8_t> text_host[2];
    Event text_ev_fmt[2], text_ev_copy[2];
    std::string h_fmt_blob;
    bool fmt_blob_on_device = false;      // d_fmt_names / d_fmt_soff hold h_fmt_blob / h_fmt_soff
    std::vector<uint32_t> h_fmt_soff;
    // pinned staging for host -> device copies of file bytes (upload_ranges)
    PinnedBuf<uint8_t> stage[kStages];
    Event stage_ev[kStages], upload_done;
    PinnedBuf<HostResults> res;     // one element, allocated by results()

    DevBuf<uint8_t> d_U, d_scratch, d_lit;
    uint64_t primary_records = 0;   // records of THIS file in the last run (stats.n_records is the sum over files after a merge)
    // several BAMs whose dictionaries differ (merge_dictionaries, host_io.hpp): hdr.refs is the MERGED dictionary in every file's
    // context; the records and the BAI of a file speak its own ids.  Empty: the file's own dictionary is the merged one.
    std::vector<int32_t> own_to_merged, merged_to_own;
    DevBuf<int32_t> d_own_to_merged;
    uint64_t index_straddler = kOffUnknown;      // index mode, open-ended batch: work-list offset of the record the next batch starts with
    const uint8_t* U() const { return d_U.p; }
    DevBuf<uint32_t> d_ent, d_nent;
    DevBuf<uint64_t> d_entry, d_exit, d_state;
    DevBuf<uint32_t> d_count, d_flag;
    DevBuf<RecDesc> d_desc;
    DevBuf<int32_t> d_rec_ref;
    DevBuf<uint64_t> d_name_hash;
    uint64_t desc_cap = 0;
    DevBuf<uint32_t> d_mate, d_n_partners, d_mate_ext;
    DevBuf<int32_t> d_ref_len;
    DevBuf<uint32_t> d_tile_base, d_tile_lo, d_tile_hi, d_active, d_slot_of, d_n_active;
    DevBuf<unsigned long long> d_scan_part;      // scratch of the multi-workgroup scans of K2 (index.hip)
    DevBuf<uint32_t> d_counters, d_span;
    DevBuf<uint32_t> d_covm, d_addm;     // per-column quantities of region/window runs with --fix-mate-overlaps
    DevBuf<DeviceFilter> d_filter;
    DevBuf<uint8_t> d_ref_sets;
    DevBuf<char> d_rg_ids;
    DevBuf<uint32_t> d_rg_off;
    DevBuf<uint16_t> d_rg_sample;
    DevBuf<IndexStats> d_stats;
    DevBuf<unsigned long long> d_tok;      // token bytes of the last inflate (accounting)
    DevBuf<SortedRegion> d_sel;
    DevBuf<uint32_t> d_sel_first;
    DevBuf<uint32_t> d_fmt_len, d_fmt_soff;
    DevBuf<uint64_t> d_fmt_off;
    DevBuf<uint8_t> d_fmt_text;
    DevBuf<char> d_fmt_names;
    // host images of the small tables (they must outlive the asynchronous copies that read them)
    std::vector<int32_t> h_ref_len;
    std::vector<uint32_t> h_tile_base_up, h_sel_first, h_rg_off;
    std::vector<SortedRegion> h_sel;
    std::vector<uint8_t> h_ref_sets;
    std::string h_rg_ids;
    DeviceFilter h_df;
    bool filter_is_simple = false;     // the -F program of the last upload_static: only operations eval_filter_simple knows

    // region / window statistics: buffers and the preprocessed range list survive between calls (a caller that asks for the
    // same BED after every run -- bench.py config 4, the CLI per batch -- pays for sorting, chunking and uploading it once)
    struct RangeCache {
        std::vector<sbx_region> ranges;
        std::vector<uint32_t> min_start;
        bool has_min_start = false, valid = false;
        size_t n_chunks = 0;
        DevBuf<RangeChunk> d_chunks;
        DevBuf<SortedRegion> d_regs;
        DevBuf<uint32_t> d_pmax, d_first, d_min_start;
        bool sorted_valid = false;
        DevBuf<uint32_t> d_nb, d_nr, d_cov, d_seen, d_thr;
        std::vector<uint32_t> h_nb, h_nr, h_seen;
    } rc;

    // window mode: the statistics of EVERY window of the resident run, computed by the first sbx_depth_window_stats call after the run
    // (one pass over the records, one reduction over the positions) and handed out contig by contig
    struct WindowCache {
        bool valid = false;
        uint64_t serial = 0;
        uint32_t window = 0, S = 0;
        std::vector<uint32_t> thr;
        std::vector<uint64_t> base, n_win;          // per contig
        std::vector<sbx_region_stats> st;           // [window id][S]
        std::vector<uint32_t> cov;                  // [window id][S][n_thr]
        DevBuf<uint64_t> d_base, d_nwin;
        DevBuf<uint32_t> d_nb, d_nr, d_cov, d_seen, d_thr;
        std::vector<uint32_t> h_nb, h_nr;
    } wc;
    uint64_t run_serial = 0;                        // counts the runs of this context (have_run = true)
    // The same selection run again (a bench's passes, a caller that re-runs with other parameters): the BAI query and the grouping of
    // its chunks into runs (build_runs: two sorts of the region list, the bins of every contig) and the read-selection table of K2 are
    // functions of (selection, index) alone and are kept.  Config 4 (200 k regions, 90 k runs): profiles/round5/README.md.
    struct RunsCache {
        bool valid = false, restricted = false;
        std::vector<sbx_region> sel;
        std::vector<FileRun> runs;
    } runs_cache;
    std::vector<sbx_region> sel_uploaded;           // the selection whose table sits in d_sel / d_sel_first
    bool sel_uploaded_valid = false;

    // result of the last sbx_parse_regions
    std::vector<sbx_region> parsed_merged, parsed_raw;
    std::vector<std::string> parsed_lines;

    // results of the last run
    bool have_run = false;
    uint32_t tile_pos = 0, n_samples_eff = 1, n_tiles = 0, n_active = 0;
    // spare position tiles behind the last position of every contig, for alignments hanging over its end; enlarged (and kept) when a
    // pass meets an alignment that reaches beyond them (run_impl); spare_of_run: what the last pass was laid out with
    uint32_t spare_tiles = 1, spare_of_run = 0;
    // > 0 while sbx_stream_base_rows is handing text out.  The one call allowed on another thread meanwhile is
    // sbx_prefetch_interval: it touches the work list, the compressed bytes and the block tables (make_resident) -- nothing the text path
    // reads (counters, slot_of, tile_base, span, the format buffers).  A RUN replaces exactly those: it refuses while text is streaming.
    std::atomic<int> text_streaming{0};
    bool span_valid = false;
    std::vector<uint32_t> h_tile_base, h_slot_of;
    sbx_run_stats stats{};

    // compute; file bytes host -> device; text device -> host.  Declared LAST: members are destroyed in reverse order, and a stream's
    // destructor waits for what is queued on it -- so every buffer and event above outlives the work that may still be using it.
    Stream stream, copy_stream, text_stream;
};

namespace sbx {

// the files of a (possibly multi-BAM) context, the primary first
inline std::vector<sbx_ctx*> files_of(sbx_ctx* c) {
    std::vector<sbx_ctx*> v{c};
    v.insert(v.end(), c->members.begin(), c->members.end());
    return v;
}

template <class F>
int guarded(sbx_ctx* c, F&& f) {
    try {
        // several contexts on several devices, driven from any thread: the device is a property of the context, not of the thread
        if (c) SBX_HIP(hipSetDevice(c->device));
        f();
        return SBX_OK;
    } catch (const Error& e) {
        if (c) { std::lock_guard<std::mutex> g(c->err_mu); c->last_error = e.what(); }
        return e.code;
    } catch (const std::exception& e) {
        if (c) { std::lock_guard<std::mutex> g(c->err_mu); c->last_error = e.what(); }
        return SBX_EINVAL;
    }
}

inline void set_err(char* err, size_t n, const std::string& m) {
    if (err && n) snprintf(err, n, "%s", m.c_str());
}

// the pinned result words of the context
inline HostResults& results(sbx_ctx* c) {
    c->res.ensure(1);
    return *c->res.p;
}

// SBX_E* code of the last sbx_open of this thread that failed (sbx_open itself returns null and a message; the standalone entry
// points built on it -- sbx_flagstat -- return the code)
extern thread_local int t_open_code;

// ---- the standalone entry points: one call opens a file, passes over it and closes it (sbx_flagstat, sbx_build_index and the
// commands of engine_store.hpp) ----

// Runs the body of an entry point; an Error or std::exception that leaves it becomes the returned code and the text in err.  What
// the body owns -- a Standalone context, an OutputGuard, device buffers -- is cleaned up while the exception unwinds it.
template <class F>
int run_entry(char* err, size_t errlen, F&& body) {
    try {
        body();
        return SBX_OK;
    } catch (const Error& e) {
        set_err(err, errlen, e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SBX_EINVAL;
    }
}

// the context of one entry point: closed when it leaves scope, or early by reset() (the batch buffers of a read pass make room)
struct Standalone {
    sbx_ctx* c = nullptr;
    Standalone() = default;
    explicit Standalone(sbx_ctx* p) : c(p) {}
    Standalone(Standalone&& o) noexcept : c(o.c) { o.c = nullptr; }
    Standalone& operator=(Standalone&& o) noexcept { reset(); c = o.c; o.c = nullptr; return *this; }
    ~Standalone() { reset(); }
    void reset() { if (c) sbx_close(c); c = nullptr; }
    sbx_ctx* operator->() const { return c; }
    sbx_ctx* get() const { return c; }
};

inline bool has_ops(const sbx_filter* filter) { return filter && filter->n_ops > 0; }

// one file, opened; a failure carries the SBX_E* code of the open
inline Standalone open_standalone(const char* path, int device) {
    const char* one[1] = {path};
    char e2[512] = {0};
    Standalone c(sbx_open(one, 1, device, e2, sizeof e2));
    if (!c.get()) throw Error(t_open_code != SBX_OK ? t_open_code : SBX_EIO, e2);
    return c;
}

// ... and set up for an index-mode pass (for_each_record_batch): every record is described; no sort order, index or read group is
// required.  filter (optional; an empty one counts as none): the -F program K2 runs, not depth's default filter.
// verdict_on_every_record: K2 leaves the filter's verdict in RecDesc::pad of every record (an empty filter admits all of them).
inline Standalone open_record_pass(const char* path, int device, const sbx_filter* filter, bool verdict_on_every_record) {
    Standalone c = open_standalone(path, device);
    c->index_mode = true;
    memset(&c->filter, 0, sizeof c->filter);
    if (has_ops(filter)) c->filter = *filter;
    c->filter_every = verdict_on_every_record;
    c->mode = SBX_MODE_BASE;
    c->fix_mate = false;
    return c;
}

// ---- argument checks with one wording ----
inline void check_level(int level) {
    if (level < -1 || level > 9) throw Error(SBX_EINVAL, "compression level must be -1 (default) or 0 .. 9");
}
inline void check_filter(const sbx_filter* filter) {
    if (filter && (filter->n_ops < 0 || filter->n_ops > SBX_FILTER_MAX_OPS)) throw Error(SBX_EINVAL, "malformed filter");
}
inline void refuse_overwrite(const char* in_path, const char* out_path) {
    if (same_file(in_path, out_path)) throw Error(SBX_EINVAL, std::string("the output would overwrite the input ") + in_path);
}

// engine_worklist.cpp
std::vector<sbx_region> sorted_regions(const std::vector<sbx_region>& sel);
std::vector<FileRun> build_runs(const sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted);
void make_resident(sbx_ctx* c, std::vector<FileRun> runs);
void inflate_worklist(sbx_ctx* c, hipEvent_t ev_mid);
void parse_header_on_device(sbx_ctx* c);
uint64_t voffset_to_stream(const sbx_ctx* c, uint64_t v, uint32_t* blk);
std::vector<uint8_t> inflate_stream_prefix(sbx_ctx* c, uint64_t n_bytes);
// engine_run.cpp
void run_impl(sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted, const std::vector<FileRun>* given_runs = nullptr);
}  // namespace sbx
