// engine_run.cpp -- the pass: K1 inflate -> K2 record index -> K3 / K7 accumulate over the resident work list (run_impl and its
// stages), the merge of several BAMs, and the ABI calls that run it: sbx_run, batches of contigs, intervals.
#include <algorithm>
#include <cstdlib>

#include "engine_ctx.hpp"

namespace sbx {

static uint32_t floor_pow2(uint32_t x) {
    uint32_t p = 1;
    while (p * 2 <= x) p *= 2;
    return p;
}

// small tables of a pass that depend on the header, the filter and the read selection only
struct StaticTables {
    uint64_t n_tiles = 0;       // position tiles of all contigs, spare tiles included
    RefTable refs{};
    RgTable rg{};
};

static StaticTables upload_static(sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted, uint32_t T) {
    StaticTables out;
    hipStream_t s = c->stream.get();
    const int32_t n_ref = (int32_t)c->hdr.refs.size();
    c->h_ref_len.assign((size_t)n_ref, 0);
    c->h_tile_base_up.assign((size_t)n_ref + 1, 0);
    uint64_t nt = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        c->h_ref_len[(size_t)r] = c->hdr.refs[(size_t)r].length;
        c->h_tile_base_up[(size_t)r] = (uint32_t)nt;
        // spare tiles per contig for alignments hanging over the contig end
        nt += ((uint64_t)std::max(0, c->hdr.refs[(size_t)r].length) + T - 1) / T + c->spare_tiles;
        if (nt > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "too many position tiles");
    }
    c->h_tile_base_up[(size_t)n_ref] = (uint32_t)nt;
    out.n_tiles = nt;
    c->d_ref_len.ensure((size_t)n_ref + 1);
    c->d_tile_base.ensure((size_t)n_ref + 1);
    if (n_ref) SBX_HIP(hipMemcpyAsync(c->d_ref_len.p, c->h_ref_len.data(), (size_t)n_ref * 4, hipMemcpyHostToDevice, s));
    SBX_HIP(hipMemcpyAsync(c->d_tile_base.p, c->h_tile_base_up.data(), ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, s));
    // -L: merged, start-sorted regions per contig for the read selection in K2
    const bool sel_same = restricted && c->sel_uploaded_valid && c->sel_uploaded.size() == sel.size() && c->d_sel.n && c->d_sel_first.n &&
                          (sel.empty() || memcmp(c->sel_uploaded.data(), sel.data(), sel.size() * sizeof(sbx_region)) == 0);
    if (restricted && !sel_same) {
        c->sel_uploaded_valid = false;
        const std::vector<sbx_region> regs = sorted_regions(sel);
        c->h_sel.clear();
        c->h_sel_first.assign((size_t)n_ref + 1, 0);
        size_t j = 0;
        for (int32_t r = 0; r < n_ref; ++r) {
            c->h_sel_first[(size_t)r] = (uint32_t)c->h_sel.size();
            bool open = false;
            while (j < regs.size() && regs[j].ref_id == (uint32_t)r) {
                if (open && c->h_sel.back().end >= regs[j].start) c->h_sel.back().end = std::max(c->h_sel.back().end, regs[j].end);
                else { c->h_sel.push_back({regs[j].start, regs[j].end, 0}); open = true; }
                ++j;
            }
        }
        c->h_sel_first[(size_t)n_ref] = (uint32_t)c->h_sel.size();
        c->d_sel.ensure(c->h_sel.size() + 1);
        c->d_sel_first.ensure((size_t)n_ref + 2);
        if (!c->h_sel.empty()) SBX_HIP(hipMemcpyAsync(c->d_sel.p, c->h_sel.data(), c->h_sel.size() * sizeof(SortedRegion), hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_sel_first.p, c->h_sel_first.data(), ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipStreamSynchronize(s));           // (the table is kept: the host copies may change before the next run needs them)
        c->sel_uploaded = sel;
        c->sel_uploaded_valid = true;
    }
    if (!c->own_to_merged.empty() && !c->d_own_to_merged.n) {
        c->d_own_to_merged.alloc(c->own_to_merged.size() + 1);
        SBX_HIP(hipMemcpyAsync(c->d_own_to_merged.p, c->own_to_merged.data(), c->own_to_merged.size() * 4, hipMemcpyHostToDevice, s));
    }
    out.refs = RefTable{c->d_ref_len.p, c->d_tile_base.p, n_ref, restricted ? c->d_sel.p : nullptr, restricted ? c->d_sel_first.p : nullptr,
                         c->own_to_merged.empty() ? nullptr : c->d_own_to_merged.p,
                         c->own_to_merged.empty() ? n_ref : (int32_t)c->own_to_merged.size()};
    // filter
    c->d_filter.ensure(1);
    DeviceFilter& df = c->h_df;
    memset(&df, 0, sizeof df);
    df.n_ops = c->filter.n_ops;
    memcpy(df.ops, c->filter.ops, sizeof(sbx_filter_op) * (size_t)c->filter.n_ops);
    memcpy(df.strings, c->filter.strings, sizeof df.strings);
    memcpy(df.regex, c->filter.regex, sizeof df.regex);
    df.n_ref = n_ref;
    c->h_ref_sets.clear();
    for (int i = 0; i < df.n_ops; ++i) {
        // ref_name / mate_ref_name == 'x' becomes a comparison of the reference id ("*" is the name of id -1)
        sbx_filter_op& o = df.ops[i];
        if (o.kind == 15 && o.field >= 4) {
            // ref_name =~ /re/: one byte per reference id + 1 ("*", the name of id -1, first)
            const sbx_regex& re = df.regex[o.value & 1];
            const size_t at0 = c->h_ref_sets.size();
            auto hit = [&](const std::string& nm) { return re_search(re, (uint32_t)nm.size(), [&](uint32_t k) { return (uint8_t)nm[k]; }) ? 1 : 0; };
            c->h_ref_sets.push_back((uint8_t)hit("*"));
            for (auto& r : c->hdr.refs) c->h_ref_sets.push_back((uint8_t)hit(r.name));
            o.kind = 16;
            o.field = (uint8_t)(o.field - 4);
            o.value = (int64_t)at0;
            continue;
        }
        if (o.kind != 11) continue;
        const size_t off = (size_t)(o.value & 0xFFFFFFFF), len = (size_t)(o.value >> 32);
        const std::string name(df.strings + std::min(off, sizeof df.strings), std::min(len, sizeof df.strings - std::min(off, sizeof df.strings)));
        const int id = name == "*" ? -1 : c->hdr.find_ref(name);
        if (id < 0 && name != "*") { o.kind = (o.cmp == 4) ? 12 : 6; continue; }     // unknown name: never equal
        o.kind = 2;
        o.field = o.field ? 4 : 0;
        o.value = id;
    }
    c->d_ref_sets.ensure(c->h_ref_sets.size() + 1);
    if (!c->h_ref_sets.empty()) SBX_HIP(hipMemcpyAsync(c->d_ref_sets.p, c->h_ref_sets.data(), c->h_ref_sets.size(), hipMemcpyHostToDevice, s));
    df.ref_sets = c->d_ref_sets.p;
    c->filter_is_simple = true;
    for (int i = 0; i < df.n_ops; ++i) c->filter_is_simple = c->filter_is_simple && filter_op_is_simple(df.ops[i].kind, df.ops[i].field);
    if (const char* e = getenv("SBX_K2_SIMPLE_FILTER")) c->filter_is_simple = c->filter_is_simple && atoi(e) != 0;      // (A/B: 0 = the interpreter always)
    SBX_HIP(hipMemcpyAsync(c->d_filter.p, &df, sizeof df, hipMemcpyHostToDevice, s));
    // read groups
    out.rg = RgTable{nullptr, nullptr, nullptr, 0, 0, 0};
    if (!c->hdr.read_groups.empty()) {
        c->h_rg_ids.clear();
        c->h_rg_off.clear();
        for (auto& g : c->hdr.read_groups) { c->h_rg_off.push_back((uint32_t)c->h_rg_ids.size()); c->h_rg_ids += g.id; c->h_rg_ids.push_back('\0'); }
        c->d_rg_ids.ensure(c->h_rg_ids.size());
        c->d_rg_off.ensure(c->h_rg_off.size());
        c->d_rg_sample.ensure(c->h_rg_off.size());
        SBX_HIP(hipMemcpyAsync(c->d_rg_ids.p, c->h_rg_ids.data(), c->h_rg_ids.size(), hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_rg_off.p, c->h_rg_off.data(), c->h_rg_off.size() * 4, hipMemcpyHostToDevice, s));
        SBX_HIP(hipMemcpyAsync(c->d_rg_sample.p, c->hdr.rg_sample.data(), c->h_rg_off.size() * 2, hipMemcpyHostToDevice, s));
        out.rg = RgTable{c->d_rg_ids.p, c->d_rg_off.p, c->d_rg_sample.p, (int32_t)c->h_rg_off.size(), 1, (uint32_t)c->h_rg_ids.size()};
    }
    if (c->index_mode) out.rg.lookup = 0;
    return out;
}

// ---- the stages of a pass (run_impl) ------------------------------------------------------------------------------------------

// Makes the work list of the selection resident: the runs the caller gives, or those of the BAI query.
// The same selection run again (RunsCache, engine_ctx.hpp) keeps its runs.
static void resolve_runs(sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted, const std::vector<FileRun>* given_runs) {
    if (given_runs) { make_resident(c, *given_runs); return; }
    const double t0 = wall_now();
    sbx_ctx::RunsCache& rcache = c->runs_cache;
    // (SBX_RUNS_CACHE=0: every run builds its work list, as a one-shot command does -- bench.py times config 4 both ways)
    const char* rc_env = getenv("SBX_RUNS_CACHE");
    if (rc_env && atoi(rc_env) == 0) { rcache.valid = false; c->sel_uploaded_valid = false; }
    const bool hit = rcache.valid && rcache.restricted == restricted && rcache.sel.size() == sel.size() &&
                     (sel.empty() || memcmp(rcache.sel.data(), sel.data(), sel.size() * sizeof(sbx_region)) == 0);
    if (!hit) {
        rcache.valid = false;
        rcache.runs = build_runs(c, sel, restricted);
        rcache.sel = sel;
        rcache.restricted = restricted;
        rcache.valid = true;
    }
    const double t1 = wall_now();
    make_resident(c, rcache.runs);
    if (getenv("SBX_TIMING")) fprintf(stderr, "[sbx] run: work list %.1f ms, resident %.1f ms\n", (t1 - t0) * 1e3, (wall_now() - t1) * 1e3);
}

// samples counted apart and positions per tile
struct PassGeometry { uint32_t S, T; };

static PassGeometry pass_geometry(const sbx_ctx* c) {
    const uint32_t S = c->combined ? 1u : (uint32_t)c->hdr.sample_names.size();
    const uint32_t T = std::max<uint32_t>(16, floor_pow2(std::max<uint32_t>(1, 1024u / std::max<uint32_t>(1, S))));
    if ((size_t)448 * S + 64 > 160u * 1024)
        throw Error(SBX_EUNSUPPORTED, "too many samples for the device path (" + std::to_string(S) + "): the counters of a position tile no longer fit "
                                      "the LDS of a compute unit; use --combined");
    return {S, T};
}

// tiles with this many records or more keep 32-bit LDS counters in K3 (debug hook: a small value sends ordinary tiles
// down that path, tests/test_gpu_depth.py)
static uint32_t deep_tile_threshold() {
    uint32_t deep_thr = kDeepTileRecords;
    if (const char* e = getenv("SBX_DEEP_TILE_RECORDS")) { const long v = atol(e); if (v >= 1 && v < (long)kDeepTileRecords) deep_thr = (uint32_t)v; }
    return deep_thr;
}

static IndexArgs fill_index_args(sbx_ctx* c, const RefTable& refs, const RgTable& rg, uint32_t T, bool entries_given) {
    IndexArgs a{};
    a.U = c->d_U.p;
    a.u_alloc = (c->wl.u_bytes + 15) & ~15ull;
    a.out_off = c->d_out_off.p; a.isize = c->d_isize.p; a.run_of = c->d_run_of.p; a.runs = c->d_runs.p;
    a.n_blocks = (uint32_t)c->wl.n_blocks();
    a.inflate_status = c->d_status.p;
    a.entry_in = entries_given ? c->d_entry.p : nullptr;
    a.entry = c->d_entry.p; a.exit_ = c->d_exit.p; a.count = c->d_count.p;
    a.state = c->d_state.p; a.scratch = c->d_lit.p;
    a.refs = refs; a.filt = c->d_filter.p; a.rg = rg; a.tile_pos = T;
    a.simple_filter = c->filter_is_simple ? 1u : 0u;
    a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.name_hash = c->fix_mate ? c->d_name_hash.p : nullptr;
    a.desc_cap = c->desc_cap;
    a.tile_lo = c->d_tile_lo.p; a.tile_hi = c->d_tile_hi.p; a.stats = c->d_stats.p; a.flags = c->d_flag.p;
    a.scan_part = c->d_scan_part.p;
    a.own_ref = c->own_ref; a.own_beg = c->own_beg; a.own_end = c->own_end;
    a.filter_every = c->filter_every ? 1u : 0u;
    return a;
}

// SBX_DEBUG: the chain around the first inconsistent block
static void dump_chain_around(sbx_ctx* c, uint32_t first_bad) {
    const WorkList& w = c->wl;
    const uint32_t nb = (uint32_t)w.n_blocks();
    const uint32_t b0 = first_bad >= 2 ? first_bad - 2 : 0, b1 = std::min<uint32_t>(nb, first_bad + 3);
    std::vector<uint64_t> he(b1 - b0), hx(b1 - b0);
    std::vector<uint32_t> hc(b1 - b0);
    SBX_HIP(hipMemcpy(he.data(), c->d_entry.p + b0, (b1 - b0) * 8ull, hipMemcpyDeviceToHost));
    SBX_HIP(hipMemcpy(hx.data(), c->d_exit.p + b0, (b1 - b0) * 8ull, hipMemcpyDeviceToHost));
    SBX_HIP(hipMemcpy(hc.data(), c->d_count.p + b0, (b1 - b0) * 4ull, hipMemcpyDeviceToHost));
    for (uint32_t b = b0; b < b1; ++b)
        fprintf(stderr, "[sbx]     block %u: out_off=%llu isize=%u entry=%lld exit=%lld count=%u\n", b, (unsigned long long)w.out_off[b], w.isize[b],
                (long long)he[b - b0], (long long)hx[b - b0], hc[b - b0]);
}

// A guessed entry was wrong (or a block holds no record start).  Wrong guesses are isolated, so they are repaired in parallel
// first: every block that is not entered where its predecessor was left is walked again from there, round after round until
// nothing changes.  What is left after a few rounds (a long stretch of blocks without record starts, a corrupt file) -- and the
// test hook -- goes to the serial repair, which follows the chain from the first inconsistent block on.  Returns the blocks walked again.
// Whatever the rounds produce is only a proposal: the pass is repeated with these entries, and the chain check of that pass
// (k_check_scan, every block against its predecessor) is what accepts or rejects it.
static uint32_t repair_chain(sbx_ctx* c, const IndexArgs& a, uint32_t first_bad, bool forced) {
    hipStream_t s = c->stream.get();
    HostResults& R = results(c);
    uint32_t* d_rewalked = c->d_flag.p + kFlagRewalked;
    uint32_t n_rewalked = 0;
    bool settled = false;
    if (!forced) {
        for (int round = 0; round < 8 && !settled; ++round) {
            SBX_HIP(hipMemsetAsync(d_rewalked, 0, 4, s));
            launch_rewalk_mismatched(a, d_rewalked, s);
            SBX_HIP(hipMemcpyAsync(&R.n_rewalked, d_rewalked, 4, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            n_rewalked += R.n_rewalked;
            settled = R.n_rewalked == 0 && round > 0;
            if (R.n_rewalked == 0) break;
        }
    }
    if (!settled) {
        SBX_HIP(hipMemsetAsync(d_rewalked, 0, 4, s));
        launch_chain_repair(c->d_U.p, c->d_out_off.p, c->d_isize.p, c->d_run_of.p, c->d_runs.p, a.n_blocks, first_bad, c->d_entry.p, c->d_exit.p,
                            c->d_count.p, d_rewalked, s);
        SBX_HIP(hipMemcpyAsync(&R.n_rewalked, d_rewalked, 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        n_rewalked += R.n_rewalked;
    }
    return n_rewalked;
}

static IndexStats sum_index_stats(const IndexStats* st) {
    IndexStats ist{};
    for (uint32_t k = 0; k < kIndexStatSlots; ++k) {
        const IndexStats& x = st[k];
        ist.n_records += x.n_records; ist.n_admitted += x.n_admitted; ist.n_bad += x.n_bad; ist.n_unknown_rg += x.n_unknown_rg;
        ist.adm_seq_bytes += x.adm_seq_bytes; ist.adm_qual_bytes += x.adm_qual_bytes;
        ist.max_span = std::max(ist.max_span, x.max_span);
    }
    return ist;
}

struct IndexResult {
    uint64_t n_records;         // of the record chain
    IndexStats ist;             // of the describe pass, summed over its slots
    uint32_t n_active, n_deep;  // tiles with records; those of them with deep_thr records or more
    uint32_t n_rewalked;        // blocks the repairs walked again
};

// K2: record chain, descriptors, tile ranges and the list of active tiles.  The pass is launched again when the chain was guessed
// wrong (after repair_chain, with the entries given), when the descriptor array was too small, and when an alignment reaches
// beyond the spare tiles of its contig (then `tab` is laid out again).  t_index times the first attempt.
static IndexResult index_pass(sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted, uint32_t T, uint32_t deep_thr,
                              StaticTables* tab, EventTimer* t_index) {
    hipStream_t s = c->stream.get();
    HostResults& R = results(c);
    const WorkList& w = c->wl;
    const uint32_t nb = (uint32_t)w.n_blocks();
    auto ensure_tiles = [&] {
        c->d_tile_lo.ensure((size_t)tab->n_tiles + 1);
        c->d_tile_hi.ensure((size_t)tab->n_tiles + 1);
        c->d_active.ensure((size_t)tab->n_tiles + 1);
        c->d_slot_of.ensure((size_t)tab->n_tiles + 1);
    };
    c->d_entry.ensure(nb + 1);
    c->d_exit.ensure(nb + 1);
    c->d_state.ensure(nb + 1);
    c->d_count.ensure(nb + 1);
    c->d_flag.ensure(kFlagWords);
    ensure_tiles();
    c->d_n_active.ensure(4);
    c->d_scan_part.ensure(kScanPartWords);
    c->d_stats.ensure(kIndexStatSlots);
    // descriptor capacity: sized for records of >= 160 bytes on average; K2 reports an overflow and the pass is repeated
    // with the exact number (short-read fixtures, amplicon data with tiny records)
    uint64_t want_cap = std::max<uint64_t>(c->desc_cap, w.u_bytes / 160 + 4096);
    if (want_cap > c->desc_cap) want_cap += (uint64_t)((double)want_cap * devbuf_slack_pct().load(std::memory_order_relaxed) / 100.0);
    const bool dbg = getenv("SBX_DEBUG") != nullptr;
    const char* force = getenv("SBX_FORCE_REPAIR");   // debug hook (tests/test_gpu_repair.py)
    uint32_t n_rewalked = 0;
    uint64_t n_records = 0;
    bool entries_given = false, spare_retried = false;
    t_index->start(s);
    for (int attempt = 0;; ++attempt) {
        if (attempt > 4) throw Error(SBX_EFORMAT, "BAM record chain does not converge");
        if (want_cap > 0xFFFFFFF0ull) throw Error(SBX_EUNSUPPORTED, "more than 2^32 records in one batch");
        if (want_cap > c->desc_cap) {
            c->d_desc.release(); c->d_rec_ref.release();
            c->d_desc.alloc((size_t)want_cap + 64);
            c->d_rec_ref.alloc((size_t)want_cap + 64);
            if (c->d_name_hash.n) { c->d_name_hash.release(); }
            c->desc_cap = want_cap;
        }
        if (c->fix_mate) c->d_name_hash.ensure((size_t)c->desc_cap + 64);
        const uint64_t nt = tab->n_tiles;
        SBX_HIP(hipMemsetAsync(c->d_tile_lo.p, 0xFF, (size_t)nt * 4, s));
        SBX_HIP(hipMemsetAsync(c->d_tile_hi.p, 0, (size_t)nt * 4, s));
        SBX_HIP(hipMemsetAsync(c->d_stats.p, 0, sizeof(IndexStats) * kIndexStatSlots, s));
        SBX_HIP(hipMemsetAsync(c->d_state.p, 0, ((size_t)nb + 1) * 8, s));
        SBX_HIP(hipMemsetAsync(c->d_flag.p + kFlagFirstBad, 0xFF, (kFlagDescOverflow - kFlagFirstBad) * 4, s));
        SBX_HIP(hipMemsetAsync(c->d_flag.p + kFlagDescOverflow, 0, (kFlagStraddler - kFlagDescOverflow) * 4, s));
        SBX_HIP(hipMemsetAsync(c->d_flag.p + kFlagStraddler, 0xFF, 8, s));
        const IndexArgs a = fill_index_args(c, tab->refs, tab->rg, T, entries_given);
        launch_index_blocks(a, s);
        launch_tile_compact(c->d_tile_lo.p, c->d_tile_hi.p, (uint32_t)nt, deep_thr, c->d_active.p, c->d_slot_of.p, c->d_n_active.p,
                            c->d_scan_part.p, s);
        if (attempt == 0) t_index->stop(s);
        R.last_state = 0;
        SBX_HIP(hipMemcpyAsync(R.flags, c->d_flag.p, sizeof R.flags, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(&R.n_active, c->d_n_active.p, 8, hipMemcpyDeviceToHost, s));      // n_active, n_deep
        SBX_HIP(hipMemcpyAsync(R.st, c->d_stats.p, sizeof(IndexStats) * kIndexStatSlots, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipMemcpyAsync(R.tok_bytes, c->d_tok.p, 64 * 8, hipMemcpyDeviceToHost, s));
        if (nb) SBX_HIP(hipMemcpyAsync(&R.last_state, c->d_state.p + (nb - 1), 8, hipMemcpyDeviceToHost, s));
        if (c->index_mode) SBX_HIP(hipMemcpyAsync(&R.straddler, c->d_flag.p + kFlagStraddler, 8, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));                            // ---- host synchronisation 1 of 2 ----
        if (R.flags[kFlagFailedInflate] != 0xFFFFFFFFu) {
            const uint32_t b = R.flags[kFlagFailedInflate];
            uint32_t st = 0;
            SBX_HIP(hipMemcpy(&st, c->d_status.p + b, 4, hipMemcpyDeviceToHost));
            throw Error(SBX_EFORMAT, "Error inflating BGZF block starting from offset " + std::to_string(c->blocks.coffset[w.file_blk[b]]) + ": " +
                                         inflate_status_string(st));
        }
        n_records = R.last_state & ((1ull << 62) - 1);
        uint32_t first_bad = R.flags[kFlagFirstBad];
        bool forced = false;
        if (force && attempt == 0 && !entries_given) { const uint32_t f = (uint32_t)atoi(force); if (f < first_bad && f < nb) { first_bad = f; forced = true; } }
        const bool bad_chain = first_bad != 0xFFFFFFFFu && first_bad < nb;
        if (dbg) fprintf(stderr, "[sbx]   index attempt %d: records=%llu first_bad=%u overflow=%u cap=%llu\n", attempt,
                         (unsigned long long)n_records, first_bad, R.flags[kFlagDescOverflow], (unsigned long long)c->desc_cap);
        if (dbg && bad_chain) dump_chain_around(c, first_bad);
        if (bad_chain) {
            // launch again with the entries the repair proposes; a chain that is still inconsistent then is a corrupt file
            if (entries_given && !forced) throw Error(SBX_EFORMAT, "BAM record chain is broken (truncated or corrupt record)");
            n_rewalked += repair_chain(c, a, first_bad, forced);
            entries_given = true;
            continue;
        }
        if (R.flags[kFlagDescOverflow]) { want_cap = n_records + 1024; continue; }
        if (R.st[0].over_tiles && !c->index_mode) {
            // an admitted alignment reaches beyond the spare tiles of its contig (the reference prints every column a read covers,
            // pileup.d:345-397): lay the tiles out with room for it and repeat the pass -- the chain is known by now
            if (spare_retried) throw Error(SBX_EFORMAT, "internal error: alignments beyond the enlarged spare tiles");
            spare_retried = true;
            const uint64_t want = (uint64_t)c->spare_tiles + R.st[0].over_tiles;
            if (want > 0x7FFFFFFFull / T + 2) throw Error(SBX_EFORMAT, "malformed BAM record (an alignment ends beyond position 2^31)");
            c->spare_tiles = (uint32_t)want;
            *tab = upload_static(c, sel, restricted, T);
            ensure_tiles();
            entries_given = true;
            attempt = 0;
            continue;
        }
        break;
    }
    c->spare_of_run = c->spare_tiles;
    return {n_records, sum_index_stats(R.st), R.n_active, R.n_deep, n_rewalked};
}

// what K3 left per active tile
struct CounterLayout {
    bool want_span;         // d_span holds the positions' spans
    size_t per_tile;        // words of d_counters
};

// K3, or with -m K7: the counters of the active tiles.  t_acc times the kernels (and, with -m, the host's look at the partner counts).
static CounterLayout accumulate_pass(sbx_ctx* c, PassGeometry g, const IndexResult& ix, uint32_t deep_thr, EventTimer* t_acc) {
    hipStream_t s = c->stream.get();
    HostResults& R = results(c);
    const uint32_t S = g.S, T = g.T, n_active = ix.n_active;
    const uint64_t n_records = ix.n_records;
    const int32_t n_ref = (int32_t)c->hdr.refs.size();
    const bool want_span = c->min_bq > 0 || (c->fix_mate && c->mode != SBX_MODE_BASE);
    // region / window statistics are sums over {bases counted, depth} per position (reduce.hip): without -m, for a single file and
    // without a tile of 2^16 records or more K3 writes that one word per position instead of seven counters (SBX_COMPACT=0: never)
    static const bool compact_ok = [] { const char* e = getenv("SBX_COMPACT"); return !e || atoi(e) != 0; }();
    const bool compact = compact_ok && c->mode != SBX_MODE_BASE && !c->fix_mate && !c->in_group && ix.n_deep == 0;
    c->compact_counters = compact;
    const size_t per_tile = compact ? (size_t)T * S : (size_t)T * S * SBX_NCOUNTERS;
    c->d_counters.ensure((size_t)n_active * per_tile + 4);
    if (want_span) c->d_span.ensure((size_t)n_active * T + 4);
    if (c->fix_mate) {
        c->d_mate.ensure((size_t)n_records + 64);
        c->d_n_partners.ensure((size_t)n_records + 64);
        SBX_HIP(hipMemsetAsync(c->d_mate.p, 0xFF, (size_t)n_records * 4, s));
        SBX_HIP(hipMemsetAsync(c->d_n_partners.p, 0, (size_t)n_records * 4, s));
    }
    t_acc->start(s);
    if (c->fix_mate) {
        launch_find_mates(c->U(), c->d_desc.p, c->d_name_hash.p, c->d_rec_ref.p, n_records, c->d_mate.p, c->d_n_partners.p, s);
        launch_max_u32(c->d_n_partners.p, n_records, c->d_flag.p + kFlagMaxPartners, s);
        SBX_HIP(hipMemcpyAsync(&R.max_partners, c->d_flag.p + kFlagMaxPartners, 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        const char* many_msg = "--fix-mate-overlaps: four or more overlapping records with the same name cover one position, or one record "
                               "overlaps four or more records with the same name wherever they lie (or, in region / window mode, a record "
                               "overlaps two or more such records); the reference's result then depends on the hash order of unrelated "
                               "reads (depth.d:343-377) and is not on the device path";
        // bit 31: some record has a partner AND overlaps a same-name record of another sample.  In the reference's column that record
        // can sort between the partners, which then are no neighbours and do not pair (depth.d:343-377)
        if (R.max_partners & 0x80000000u)
            throw Error(SBX_EUNSUPPORTED, "--fix-mate-overlaps: overlapping records with the same name belong to different samples and two "
                                          "of them to the same one; whether the reference pairs those two depends on the order of the "
                                          "column (depth.d:343-377) and is not on the device path");
        if (R.max_partners > 1 && c->mode != SBX_MODE_BASE) throw Error(SBX_EUNSUPPORTED, many_msg);
        if (c->mode == SBX_MODE_BASE) {
            const bool multi = R.max_partners > 1;
            if (multi) {
                // groups of more than two same-name records: list up to three partners per record
                c->d_mate_ext.ensure(3 * (size_t)n_records + 64);
                SBX_HIP(hipMemsetAsync(c->d_mate_ext.p, 0xFF, 3 * (size_t)n_records * 4, s));
                SBX_HIP(hipMemsetAsync(c->d_n_partners.p, 0, (size_t)n_records * 4, s));
                launch_find_partners(c->U(), c->d_desc.p, c->d_name_hash.p, c->d_rec_ref.p, n_records, c->d_mate_ext.p, c->d_n_partners.p, s);
            }
            launch_accumulate_mates(c->U(), c->d_desc.p, c->d_mate.p, c->d_tile_lo.p, c->d_tile_hi.p, c->d_active.p, n_active,
                                    c->d_tile_base.p, n_ref, T, S, c->min_bq, multi ? c->d_mate_ext.p : nullptr, c->d_n_partners.p,
                                    c->d_flag.p + kFlagMatesOverflow, c->d_counters.p, want_span ? c->d_span.p : nullptr, s);
            if (multi) {
                SBX_HIP(hipMemcpyAsync(&R.max_partners, c->d_flag.p + kFlagMatesOverflow, 4, hipMemcpyDeviceToHost, s));
                SBX_HIP(hipStreamSynchronize(s));
                if (R.max_partners) throw Error(SBX_EUNSUPPORTED, many_msg);
            }
        } else {
            // region / window: the statistics come from per-column quantities, not from the base counters
            c->d_covm.ensure((size_t)n_active * T * S + 1);
            c->d_addm.ensure((size_t)n_active * T * S + 1);
            if (n_active) SBX_HIP(hipMemsetAsync(c->d_counters.p, 0, (size_t)n_active * per_tile * 4, s));
            launch_mates_columns(c->U(), c->d_desc.p, c->d_mate.p, c->d_tile_lo.p, c->d_tile_hi.p, c->d_active.p, n_active,
                                 c->d_tile_base.p, n_ref, T, S, c->min_bq, c->d_covm.p, c->d_addm.p, c->d_span.p, s);
        }
    } else
        launch_accumulate(c->U(), c->d_desc.p, c->d_tile_lo.p, c->d_tile_hi.p, c->d_active.p, n_active, ix.n_deep, deep_thr, c->d_tile_base.p,
                          n_ref, T, S, c->min_bq, c->d_counters.p, want_span ? c->d_span.p : nullptr, s, compact);
    t_acc->stop(s);
    return {want_span, per_tile};
}

struct PassTimers { EventTimer all, inflate, inflate_mid, index, accumulate; };      // inflate_mid.b: between K1a and K1b

// the results of the pass for the queries that follow, and its statistics
static void record_run_stats(sbx_ctx* c, PassGeometry g, uint64_t n_tiles, const IndexResult& ix, CounterLayout cl, PassTimers& t) {
    const WorkList& w = c->wl;
    const uint32_t nb = (uint32_t)w.n_blocks();
    const IndexStats& ist = ix.ist;
    c->h_tile_base = c->h_tile_base_up;
    c->tile_pos = g.T;
    c->n_samples_eff = g.S;
    c->n_tiles = (uint32_t)n_tiles;
    c->n_active = ix.n_active;
    c->span_valid = cl.want_span;
    c->stats.ms_inflate = t.inflate.ms();
    {
        float f = 0;
        SBX_HIP(hipEventElapsedTime(&f, t.inflate.a, t.inflate_mid.b));
        c->stats.ms_huffman = f;
        c->stats.ms_lz77 = c->stats.ms_inflate - f;
    }
    c->stats.ms_index = t.index.ms();
    c->stats.ms_accumulate = t.accumulate.ms();
    c->stats.ms_total = t.all.ms();
    c->stats.n_records = ist.n_records;
    c->stats.n_admitted = ist.n_admitted;
    c->stats.n_malformed = ist.n_bad;
    c->stats.n_bgzf_blocks = nb;
    c->stats.n_runs = w.runs.size();
    c->stats.uploaded_bytes = w.comp_bytes;
    {
        uint64_t cb = 0;
        for (auto& r : w.runs) cb += c->blocks.comp_off[r.blk1 - 1] + c->blocks.comp_len[r.blk1 - 1] + 8 - c->blocks.coffset[r.blk0];
        c->stats.compressed_bytes = cb;
    }
    c->stats.uncompressed_bytes = w.u_bytes;
    c->stats.counter_bytes = (uint64_t)ix.n_active * cl.per_tile * 4 + (cl.want_span ? (uint64_t)ix.n_active * g.T * 4 : 0);
    c->stats.token_bytes = 0;
    for (int k = 0; k < 64; ++k) c->stats.token_bytes += results(c).tok_bytes[k];
    c->stats.max_alignment_span = ist.max_span;
    c->stats.accumulate_read_bytes = 32ull * ist.n_records + ist.adm_seq_bytes + (c->min_bq > 0 || c->fix_mate ? ist.adm_qual_bytes : 0);
    c->stats.covered_positions = (uint64_t)ix.n_active * g.T;
    c->stats.launches_inflate = 1;
    c->stats.launches_index = 2 + (ix.n_rewalked ? 2 : 0);
    if (getenv("SBX_DEBUG"))
        fprintf(stderr, "[sbx] blocks=%u runs=%zu records=%llu rewalked_blocks=%u tiles=%llu active=%u T=%u\n", nb, w.runs.size(),
                (unsigned long long)ix.n_records, ix.n_rewalked, (unsigned long long)n_tiles, ix.n_active, g.T);
    c->stats.launches_accumulate = 1;
    if (getenv("SBX_TIMING")) fprintf(stderr, "[sbx] hipMalloc/hipFree so far: %.3f s\n", alloc_seconds());
    c->have_run = true;
    ++c->run_serial;
}

// The whole device pipeline for the reads selected by `sel` (restricted == false: every read of the file).
void run_impl(sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted, const std::vector<FileRun>* given_runs) {
    if (!c->index_mode) {
        if (c->hdr.sorting_order != "coordinate") throw Error(SBX_ENOTSORTED, "All files must be coordinate-sorted");
        if (!c->has_index) throw Error(SBX_ENOINDEX, "All files must be indexed");
    }
    SBX_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream.get();
    c->have_run = false;
    c->stats = sbx_run_stats{};

    // ---- work list, tables, compressed bytes ----
    resolve_runs(c, sel, restricted, given_runs);
    c->stats.ms_h2d = c->upload_ms.load(std::memory_order_relaxed);      // (the upload may have been a prefetch on another thread)
    PassTimers t;
    t.all.start(s);

    // ---- K1 ----
    t.inflate.start(s);
    inflate_worklist(c, t.inflate_mid.b);
    t.inflate.stop(s);

    // ---- K2 ----
    const PassGeometry g = pass_geometry(c);
    StaticTables tab = upload_static(c, sel, restricted, g.T);
    const uint32_t deep_thr = deep_tile_threshold();
    const IndexResult ix = index_pass(c, sel, restricted, g.T, deep_thr, &tab, &t.index);
    if (ix.ist.n_records != ix.n_records)
        throw Error(SBX_EFORMAT, "internal error: record chain (" + std::to_string(ix.n_records) + ") and describe pass (" +
                                     std::to_string(ix.ist.n_records) + ") disagree on the number of records");
    if (c->index_mode) {              // the descriptors are the result
        c->primary_records = ix.n_records;
        c->index_straddler = results(c).straddler;
        c->stats.n_records = ix.ist.n_records;
        c->stats.n_bgzf_blocks = c->wl.n_blocks();
        c->stats.ms_inflate = t.inflate.ms();
        c->stats.ms_index = t.index.ms();
        return;
    }
    if (ix.ist.n_unknown_rg)
        throw Error(SBX_ERG, "error in read: read group is not present in the header (" + std::to_string(ix.ist.n_unknown_rg) + " reads)");
    if (ix.ist.n_bad)
        throw Error(SBX_EFORMAT, "malformed BAM record (" + std::to_string(ix.ist.n_bad) + " records whose lengths are inconsistent with block_size, "
                                 "whose reference id is out of range, or which start beyond the end of their contig)");

    // ---- K3 ----
    const CounterLayout cl = accumulate_pass(c, g, ix, deep_thr, &t.accumulate);
    t.all.stop(s);
    c->h_slot_of.resize((size_t)tab.n_tiles);
    if (tab.n_tiles) SBX_HIP(hipMemcpyAsync(c->h_slot_of.data(), c->d_slot_of.p, (size_t)tab.n_tiles * 4, hipMemcpyDeviceToHost, s));
    SBX_HIP(hipStreamSynchronize(s));                                // ---- host synchronisation 2 of 2 ----

    record_run_stats(c, g, tab.n_tiles, ix, cl, t);
}

// Several BAMs: every file has been through the pipeline on its own; the per-position results are sums over the
// files (the pileup of the merged stream is the union of the reads), so the primary's tile set becomes the union
// of the files' tile sets with the counters added up.  Per-read work that needs a file's records (read counts of
// regions / windows) is done file by file at query time.
static void merge_members(sbx_ctx* c) {
    if (c->members.empty()) return;
    SBX_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream.get();
    const auto files = files_of(c);
    const uint32_t T = c->tile_pos, S = c->n_samples_eff;
    const size_t nt = c->h_slot_of.size();
    for (sbx_ctx* m : files)
        if (m->tile_pos != T || m->n_samples_eff != S || m->h_slot_of.size() != nt) throw Error(SBX_EINVAL, "internal: tile grids differ");
    std::vector<uint32_t> slot(nt, 0xFFFFFFFFu);
    uint32_t n_active = 0;
    for (size_t t = 0; t < nt; ++t) {
        bool on = false;
        for (sbx_ctx* m : files) on |= m->h_slot_of[t] != 0xFFFFFFFFu;
        if (on) slot[t] = n_active++;
    }
    const size_t per_tile = (size_t)T * S * SBX_NCOUNTERS;
    const bool region_m = c->fix_mate && c->mode != SBX_MODE_BASE;
    DevBuf<uint32_t> d_slot(nt + 1), cnt((size_t)n_active * per_tile + 4), spn, covm, addm;
    if (nt) SBX_HIP(hipMemcpyAsync(d_slot.p, slot.data(), nt * 4, hipMemcpyHostToDevice, s));
    SBX_HIP(hipMemsetAsync(cnt.p, 0, cnt.bytes(), s));
    if (c->span_valid) { spn.alloc((size_t)n_active * T + 4); SBX_HIP(hipMemsetAsync(spn.p, 0, spn.bytes(), s)); }
    if (region_m) {
        covm.alloc((size_t)n_active * T * S + 1); addm.alloc((size_t)n_active * T * S + 1);
        SBX_HIP(hipMemsetAsync(covm.p, 0, covm.bytes(), s));
        SBX_HIP(hipMemsetAsync(addm.p, 0, addm.bytes(), s));
    }
    sbx_run_stats sum{};
    for (sbx_ctx* m : files) {
        SBX_HIP(hipStreamSynchronize(m->stream.get()));
        if (m->compact_counters) throw Error(SBX_EINVAL, "internal: a member file ran with compact counters");
        launch_merge_tiles(m->d_counters.p, m->d_active.p, m->n_active, d_slot.p, (uint32_t)per_tile, cnt.p, s);
        if (c->span_valid) launch_merge_tiles(m->d_span.p, m->d_active.p, m->n_active, d_slot.p, T, spn.p, s);
        if (region_m) {
            launch_merge_tiles(m->d_covm.p, m->d_active.p, m->n_active, d_slot.p, T * S, covm.p, s);
            launch_merge_tiles(m->d_addm.p, m->d_active.p, m->n_active, d_slot.p, T * S, addm.p, s);
        }
        const sbx_run_stats& a = m->stats;
        sum.ms_inflate += a.ms_inflate; sum.ms_index += a.ms_index; sum.ms_accumulate += a.ms_accumulate; sum.ms_total += a.ms_total;
        sum.ms_h2d += a.ms_h2d; sum.ms_huffman += a.ms_huffman; sum.ms_lz77 += a.ms_lz77;
        sum.n_records += a.n_records; sum.n_admitted += a.n_admitted; sum.n_bgzf_blocks += a.n_bgzf_blocks;
        sum.compressed_bytes += a.compressed_bytes; sum.uncompressed_bytes += a.uncompressed_bytes;
        sum.accumulate_read_bytes += a.accumulate_read_bytes; sum.token_bytes += a.token_bytes;
        sum.max_alignment_span = std::max(sum.max_alignment_span, a.max_alignment_span);
        sum.launches_inflate += a.launches_inflate; sum.launches_index += a.launches_index; sum.launches_accumulate += a.launches_accumulate;
    }
    SBX_HIP(hipStreamSynchronize(s));
    // the primary now answers for the merged tile set (its own per-file results were folded in above)
    c->primary_records = c->stats.n_records;
    std::swap(c->d_counters, cnt);
    if (c->span_valid) std::swap(c->d_span, spn);
    if (region_m) { std::swap(c->d_covm, covm); std::swap(c->d_addm, addm); }
    std::swap(c->d_slot_of, d_slot);
    c->h_slot_of = slot;
    c->n_active = n_active;
    sum.counter_bytes = (uint64_t)n_active * per_tile * 4;
    sum.covered_positions = (uint64_t)n_active * T;
    c->stats = sum;
}

static void run_files(sbx_ctx* c, const std::vector<sbx_region>& sel, bool restricted) {
    if (c->text_streaming.load() > 0)
        throw Error(SBX_EINVAL, "a run was started while sbx_stream_base_rows is handing out text of this context (only sbx_prefetch_interval may run next to it)");
    const auto files = files_of(c);
    for (sbx_ctx* m : files) run_impl(m, sel, restricted);
    // several files share one tile grid: a file that had to enlarge its spare tiles (run_impl) makes the others follow
    for (bool again = files.size() > 1; again;) {
        again = false;
        uint32_t spare = 1;
        for (sbx_ctx* m : files) spare = std::max(spare, m->spare_tiles);
        for (sbx_ctx* m : files)
            if (m->spare_of_run != spare) { m->spare_tiles = spare; run_impl(m, sel, restricted); again = true; }
    }
    if (c->fix_mate && files.size() > 1) {
        // The reference pairs same-name, same-sample records of a column across files (it merges the files before the pileup,
        // multireader.d:265-268, depth.d:338-377); the files went through the pipeline one by one and were paired within themselves.
        // That is the same thing unless such a pair exists -- which is checked here, and refused rather than printed differently.
        hipStream_t s = c->stream.get();
        uint32_t* d_hit = c->d_flag.p + kFlagCrossFile;
        SBX_HIP(hipSetDevice(c->device));
        for (sbx_ctx* m : files) SBX_HIP(hipStreamSynchronize(m->stream.get()));
        SBX_HIP(hipMemsetAsync(d_hit, 0, 4, s));
        for (size_t x = 0; x < files.size(); ++x)
            for (size_t y = x + 1; y < files.size(); ++y) {
                sbx_ctx *a = files[x], *b = files[y];
                launch_cross_file_mates(a->U(), a->d_desc.p, a->d_name_hash.p, a->d_rec_ref.p, a->stats.n_records, b->U(), b->d_desc.p,
                                        b->d_name_hash.p, b->d_rec_ref.p, b->stats.n_records, (uint32_t)b->stats.max_alignment_span,
                                        d_hit, s);
            }
        uint32_t hit = 0;
        SBX_HIP(hipMemcpyAsync(&hit, d_hit, 4, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        if (hit)
            throw Error(SBX_EUNSUPPORTED, "--fix-mate-overlaps with several BAM files: overlapping records with the same name and sample lie in "
                                          "different files; the reference pairs them across files (depth.d:338-377 on the merged stream), the "
                                          "device path pairs within a file -- merge the files first");
    }
    merge_members(c);
    ++c->run_serial;
}

}  // namespace sbx

extern "C" {

int sbx_run(sbx_ctx* c) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        run_files(c, c->regions, !c->regions.empty());
    });
}

// ---- streaming over contigs -----------------------------------------------------------------------
// BGZF block range [b0, b1) holding every read of contig r (from the BAI; empty contigs: b0 == b1)
static void contig_blocks(sbx_ctx* c, uint32_t r, uint32_t* b0, uint32_t* b1) {
    *b0 = *b1 = 0;
    if (!c->merged_to_own.empty()) {       // (the index speaks the file's own reference ids)
        if (r >= c->merged_to_own.size() || c->merged_to_own[r] < 0) return;
        r = (uint32_t)c->merged_to_own[r];
    }
    if (r >= c->bai.refs.size()) return;
    std::vector<sbx_region> whole{{r, 0u, 0x7FFFFFFFu}};
    uint64_t vbeg = ~0ull, vend = 0;
    for (auto& ch : group_chunks(c->bai, whole)) { vbeg = std::min(vbeg, ch.beg); vend = std::max(vend, ch.end); }
    if (vbeg >= vend) return;
    const auto& co = c->blocks.coffset;
    const uint32_t nb = (uint32_t)c->blocks.size();
    size_t i0 = (size_t)(std::lower_bound(co.begin(), co.end(), vbeg >> 16) - co.begin());
    size_t i1 = (size_t)(std::lower_bound(co.begin(), co.end(), vend >> 16) - co.begin());
    if (i0 >= nb) return;
    if (i1 < nb && (vend & 0xFFFF)) ++i1;
    *b0 = (uint32_t)i0;
    *b1 = (uint32_t)std::min<size_t>(std::max(i1, i0 + 1), nb);
}

// estimated device bytes of a run over BGZF blocks [b0, b1) covering `positions` reference positions:
// compressed payload + inflated stream + literal and entry token streams (~2.4x) + descriptors + counter tiles
static uint64_t footprint(sbx_ctx* c, uint32_t b0, uint32_t b1, uint64_t positions) {
    if (b1 <= b0) return 0;
    const uint64_t u = c->blocks.out_off[b1] - c->blocks.out_off[b0];
    const uint64_t comp = c->preloaded ? 0 : c->blocks.coffset[b1 - 1] - c->blocks.coffset[b0] + 65536;
    const uint32_t S = c->combined ? 1u : (uint32_t)std::max<size_t>(1, c->hdr.sample_names.size());
    return comp + u + (u + 48ull * (b1 - b0)) + 4 * (u / 3 + u / 255 + 12ull * (b1 - b0)) + u / 4 + positions * (28ull * S + 4);
}

int sbx_plan_batches(sbx_ctx* c, uint64_t budget_bytes, sbx_batch* out, size_t cap, size_t* n_out) {
    return guarded(c, [&] {
        if (!c || !n_out) throw Error(SBX_EINVAL, "null argument");
        if (!c->has_index) throw Error(SBX_ENOINDEX, "All files must be indexed");
        SBX_HIP(hipSetDevice(c->device));
        if (budget_bytes == 0) {
            size_t free_b = 0, total_b = 0;
            SBX_HIP(hipMemGetInfo(&free_b, &total_b));
            // what this context already holds (the compressed file, buffers of an earlier run) is reused
            budget_bytes = (uint64_t)((double)free_b * 0.7) + c->d_U.bytes() + c->d_lit.bytes() + c->d_ent.bytes() + c->d_counters.bytes() +
                           c->d_desc.bytes() + c->d_rec_ref.bytes() + (c->preloaded ? 0 : c->d_comp.bytes());
        }
        const uint32_t n_ref = (uint32_t)c->hdr.refs.size();
        std::vector<sbx_batch> plan;
        uint32_t first = 0, lo = 0, hi = 0;       // current batch: contigs [first, r), blocks [lo, hi)
        uint64_t pos = 0;
        for (uint32_t r = 0; r < n_ref; ++r) {
            uint32_t b0, b1;
            contig_blocks(c, r, &b0, &b1);       // (several BAMs: sized by the first file times the number of files)
            const uint64_t len = (uint64_t)std::max(0, c->hdr.refs[r].length);
            uint32_t nlo = lo, nhi = hi;
            if (b1 > b0) { nlo = hi > lo ? std::min(lo, b0) : b0; nhi = hi > lo ? std::max(hi, b1) : b1; }
            if (r > first && footprint(c, nlo, nhi, pos + len) * (1 + c->members.size()) > budget_bytes) {
                plan.push_back({first, r - first, footprint(c, lo, hi, pos)});
                first = r; pos = 0;
                nlo = b0; nhi = b1;
            }
            lo = nlo; hi = nhi; pos += len;
        }
        if (n_ref > first) plan.push_back({first, n_ref - first, footprint(c, lo, hi, pos)});
        *n_out = plan.size();
        if (out) for (size_t i = 0; i < plan.size() && i < cap; ++i) out[i] = plan[i];
        if (out && plan.size() > cap) throw Error(SBX_ENOMEM, "batch array too small");
    });
}

int sbx_run_batch(sbx_ctx* c, uint32_t first_ref, uint32_t n_refs) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        if ((uint64_t)first_ref + n_refs > c->hdr.refs.size()) throw Error(SBX_EINVAL, "Invalid reference sequence index");
        std::vector<sbx_region> sel;
        if (c->regions.empty()) {
            for (uint32_t r = first_ref; r < first_ref + n_refs; ++r) sel.push_back({r, 0u, 0x7FFFFFFFu});
        } else {
            for (auto& g : c->regions)
                if (g.ref_id >= first_ref && g.ref_id < first_ref + n_refs) sel.push_back(g);
        }
        run_files(c, sel, true);
    });
}

int sbx_run_interval(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        if (ref_id >= c->hdr.refs.size()) throw Error(SBX_EINVAL, "Invalid reference sequence index");
        if (!(beg < end)) throw Error(SBX_EINVAL, "empty interval");
        std::vector<sbx_region> sel;
        if (c->regions.empty()) sel.push_back({ref_id, beg, end});
        else
            for (auto& g : c->regions)
                if (g.ref_id == ref_id && g.start < end && g.end > beg) sel.push_back({ref_id, std::max(g.start, beg), std::min(g.end, end)});
        run_files(c, sel, true);
    });
}


int sbx_run_interval_owned(sbx_ctx* c, uint32_t ref_id, uint32_t beg, uint32_t end) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        if (ref_id >= c->hdr.refs.size()) throw Error(SBX_EINVAL, "Invalid reference sequence index");
        if (!(beg < end)) throw Error(SBX_EINVAL, "empty interval");
        if (c->fix_mate) throw Error(SBX_EUNSUPPORTED, "sbx_run_interval_owned: --fix-mate-overlaps needs both mates of a pair in one run");
        std::vector<sbx_region> sel;
        if (c->regions.empty()) sel.push_back({ref_id, beg, end});
        else
            for (auto& g : c->regions)
                if (g.ref_id == ref_id && g.start < end && g.end > beg) sel.push_back({ref_id, std::max(g.start, beg), std::min(g.end, end)});
        struct Own {      // the restriction lasts for this run only
            std::vector<sbx_ctx*> f;
            ~Own() { for (sbx_ctx* m : f) m->own_ref = -1; }
        } own{files_of(c)};
        for (sbx_ctx* m : own.f) { m->own_ref = (int32_t)ref_id; m->own_beg = beg; m->own_end = end; }
        run_files(c, sel, true);
    });
}

}  // extern "C"
