// cli_sharded.hpp -- sbx-depth over several devices.
// Several devices (`--gpus N`, SBX_DEVICES=0,1,...): ONE process, one context per device, each driven by its own thread.
// The job shards by POSITION (sbx_plan_shards): outputs of disjoint position ranges are disjoint, so nothing travels between
// the devices -- every context runs its slices (sbx_run_interval: only the BGZF blocks the BAI lists for them are uploaded
// and inflated) and hands over its share:
//   base    the text of its positions, formatted on the device and streamed piece by piece (sbx_stream_base_rows) -- with -o into its
//           own byte range of the file (pwrite at the offset the measured sizes of the slices before it add up to; the devices
//           write side by side), without -o in genome order through the one output stream, slices dealt round-robin so that
//           device k + 1 computes while device k prints;
//   region  the statistics of the BED regions whose first position it owns (a region is never split);
//   window  the statistics of the windows of its slices (cuts are multiples of the window size), the first / last columns,
//           and behind a contig's end the windows that alignments hanging over it finish or leave unfinished
// -- and the printers above print from what was collected, with the reference's rules.  Option sets whose output depends on
// the order of the whole stream (`window --overlap`, `base -L`, `base -c 0`, host formatting) run on one device, as before.
// The torch.distributed driver (python -m sambamba_amd.dist_depth) keeps the RCCL all-reduce form of the north star.
#pragma once
#include <cerrno>
#include <unistd.h>

#include "cli_base.hpp"
#include "cli_stats.hpp"

namespace sbx {

constexpr uint32_t kBaiEnd = 1u << 29;       // the coordinate limit of the BAI's binning scheme
struct Sharded {
    const Options& o;
    Out& out;
    const std::vector<const char*>& paths;
    const sbx_filter& filt;
    int mode_id;
    std::vector<int> devices;
    sbx_ctx* ctx0;                               // the context opened by depth_main (on devices[0])
    const std::vector<std::string>& samples;
    std::vector<sbx_region> merged;              // -L (region mode)
    std::vector<sbx_ctx*> cx = {};
    StageSync sync{"a device of the sharded run failed"};
    std::vector<double> busy_run = {}, busy_out = {};

    // context of device k: depth_main's for k == 0, opened here (on the worker's thread, next to the others) otherwise
    sbx_ctx* context(size_t k) {
        if (k == 0) return ctx0;
        sbx_ctx* c = open_configured(paths, devices[k], filt, mode_id, o, &merged);
        sync.mark([&] { cx[k] = c; });
        return c;
    }
    // run every worker, join them all, rethrow the first failure
    template <class W> void run_workers(W&& work) {
        cx.assign(devices.size(), nullptr);
        cx[0] = ctx0;
        busy_run.assign(devices.size(), 0);
        busy_out.assign(devices.size(), 0);
        StageThreads workers(sync);
        for (size_t k = 0; k < devices.size(); ++k)
            workers.start([&, k] {
                try { work(k, context(k)); }
                catch (const Fail& f) { sync.fail(f.msg); }
                catch (const std::exception& e) { sync.fail(e.what()); }
            });
        workers.join();
        workers.regular = true;
        if (!sync.failure.empty()) throw Fail{sync.failure};
    }
    int ref_count() { sbx_header_info hi; check(ctx0, sbx_header(ctx0, &hi)); return hi.n_ref; }
    std::vector<sbx_shard> plan(uint32_t align) {
        const int n_ref = ref_count();
        std::vector<int64_t> lens((size_t)n_ref);
        for (int r = 0; r < n_ref; ++r) lens[(size_t)r] = sbx_ref_length(ctx0, r);
        size_t n = 0;
        std::vector<sbx_shard> sh((size_t)n_ref + devices.size() + 1);
        if (sbx_plan_shards(lens.data(), n_ref, (int32_t)devices.size(), align, sh.data(), sh.size(), &n) != SBX_OK) throw Fail{"internal: shard plan"};
        sh.resize(n);
        return sh;
    }
    // sbx_run_interval over [beg - slack, end (+ slack)) with the slack --fix-mate-overlaps needs in region / window mode: a read that lies
    // past the overlap with its mate is counted differently from an unpaired one (status `past`, depth.d:717-845), so the mate must be in
    // the run even when it ends before the slice.  The slack starts at one linear-index window and is raised to the longest alignment
    // the run reports -- never silently too small.
    void run_with_mate_slack(sbx_ctx* c, uint32_t ref, uint64_t beg, uint64_t end, bool both_sides) {
        if (!o.fix_mate) { check(c, sbx_run_interval(c, ref, (uint32_t)beg, (uint32_t)end)); return; }
        uint64_t slack = 16384;
        for (int attempt = 0; attempt < 4; ++attempt) {
            const uint64_t lo = beg > slack ? beg - slack : 0, hi = both_sides ? std::min<uint64_t>(end + slack, 0x7FFFFFFFull) : end;
            check(c, sbx_run_interval(c, ref, (uint32_t)lo, (uint32_t)hi));
            sbx_run_stats st;
            check(c, sbx_last_run_stats(c, &st));
            if (st.max_alignment_span <= slack) return;
            slack = (st.max_alignment_span + 16383) / 16384 * 16384;
        }
        throw Fail{"--fix-mate-overlaps: the alignments of a slice span more than " + std::to_string(slack) + " positions; run on one device"};
    }

    // ---- base ----
    // bytes of the text of a slice (the device's measuring pass; nothing is copied)
    uint64_t measure(sbx_ctx* c, const Slice& sl) {
        uint64_t total = 0;
        for_each_active_range(c, sl.ref, sl.beg, sl.print_end, [&](uint64_t b, uint64_t e) {
            size_t need = 0;
            const int rc = sbx_format_base_rows(c, sl.ref, (uint32_t)b, (uint32_t)e, o.min_cov, o.max_cov, o.annotate ? 1 : 0, nullptr, 0, &need);
            if (rc != SBX_OK && rc != SBX_ENOMEM) check(c, rc);
            total += need;
        });
        return total;
    }
    struct Sink { int fd; uint64_t off; FILE* fp; };
    static int sink_write(void* u, const char* d, size_t n) {
        Sink* k = (Sink*)u;
        if (k->fp) return fwrite(d, 1, n, k->fp) == n ? 0 : 1;
        while (n) {
            const ssize_t w = pwrite(k->fd, d, n, (off_t)k->off);
            if (w < 0) { if (errno == EINTR) continue; return 1; }
            d += w; n -= (size_t)w; k->off += (uint64_t)w;
        }
        return 0;
    }
    void stream(sbx_ctx* c, const Slice& sl, Sink* sink) { stream_base_rows(c, o, sl.ref, sl.beg, sl.print_end, sink_write, sink); }
    void base() {
        const size_t N = devices.size();
        const bool to_file = out.fp != stdout;
        // slices: a device's share cut so that every slice still fills a device once (the lane-per-block Huffman kernel takes one
        // residency however few blocks it gets) and the buffers hold a fraction of the share
        std::vector<Slice> shares;
        for (const sbx_shard& sh : plan(1024)) shares.push_back({sh.ref_id, sh.beg, sh.end, 0, (size_t)sh.shard});
        std::vector<Slice> sl = cut_slices(ctx0, shares, std::max<uint64_t>(total_positions(ctx0, ref_count()) / (4 * N), 16u << 20));
        // one output stream: deal the slices round-robin, so that the devices compute next to the one that prints
        if (!to_file) for (size_t g = 0; g < sl.size(); ++g) sl[g].owner = g % N;
        std::vector<uint64_t> size(sl.size(), 0);
        std::vector<char> measured(sl.size(), 0), written(sl.size(), 0);
        out.flush();
        fflush(out.fp);
        const uint64_t head = to_file ? (uint64_t)ftello(out.fp) : 0;
        const int fd = to_file ? fileno(out.fp) : -1;
        run_workers([&](size_t k, sbx_ctx* c) {
            for (size_t g = 0; g < sl.size(); ++g) {
                if (sl[g].owner != k) continue;
                double t0 = now();
                // (the last slice of a contig also takes the reads that START behind the contig's end, up to the index's coordinate limit)
                check(c, sbx_run_interval(c, sl[g].ref, (uint32_t)sl[g].beg, sl[g].print_end == kPrintToEnd ? kBaiEnd : (uint32_t)sl[g].end));
                busy_run[k] += now() - t0;
                Sink sink{fd, 0, to_file ? nullptr : out.fp};
                if (to_file) {
                    const uint64_t sz = measure(c, sl[g]);
                    sync.mark([&] { size[g] = sz; measured[g] = 1; });
                    if (!sync.wait_for([&] { for (size_t i = 0; i < g; ++i) if (!measured[i]) return false; return true; })) return;
                    sink.off = head;
                    for (size_t i = 0; i < g; ++i) sink.off += size[i];
                    t0 = now();
                    const uint64_t at = sink.off;
                    stream(c, sl[g], &sink);
                    if (sink.off - at != sz) throw Fail{"internal: measured " + std::to_string(sz) + " bytes of text, wrote " + std::to_string(sink.off - at)};
                } else {
                    if (!sync.wait_for([&] { for (size_t i = 0; i < g; ++i) if (!written[i]) return false; return true; })) return;
                    t0 = now();
                    stream(c, sl[g], &sink);
                    fflush(out.fp);
                }
                busy_out[k] += now() - t0;
                sync.mark([&] { written[g] = 1; });
            }
        });
        if (to_file) {
            uint64_t all = head;
            for (uint64_t x : size) all += x;
            if (fseeko(out.fp, (off_t)all, SEEK_SET) != 0) throw Fail{"cannot seek in the output file"};
        }
    }

    // ---- region ----
    void region(RegionPrinter& rp) {
        const std::vector<sbx_shard> sh = plan(1024);
        const int n_ref = ref_count();
        // a region belongs to the device that owns its first position (regions starting at or beyond the end of their contig: the owner
        // of the contig's last position; regions of zero-length contigs: device 0 -- the one-device CLI prints a row for them as well)
        auto owner = [&](const sbx_region& g) -> size_t {
            const int64_t len = sbx_ref_length(ctx0, (int)g.ref_id);
            if (len <= 0) return 0;
            const uint64_t p = std::min<uint64_t>(g.start, (uint64_t)len - 1);
            for (const sbx_shard& x : sh)
                if (x.ref_id == g.ref_id && x.beg <= p && p < x.end) return x.shard;
            return 0;
        };
        std::vector<std::vector<size_t>> ids(devices.size());
        for (size_t i = 0; i < rp.raw.size(); ++i) ids[owner(rp.raw[i])].push_back(i);
        rp.prepare();
        run_workers([&](size_t k, sbx_ctx* c) {
            // reads are selected against ALL merged regions (a mate that reaches the pileup through a neighbour's region must still pair,
            // depth.d:717-758), but fetched only for the hull of the owned regions of a contig, widened by the mate slack on each side
            for (int r = 0; r < n_ref; ++r) {
                std::vector<size_t> mine;
                uint64_t lo = ~0ULL, hi_ = 0;
                for (size_t i : ids[k])
                    if ((int)rp.raw[i].ref_id == r) { mine.push_back(i); lo = std::min<uint64_t>(lo, rp.raw[i].start); hi_ = std::max<uint64_t>(hi_, rp.raw[i].end); }
                if (mine.empty()) continue;
                if (hi_ <= lo) hi_ = lo + 1;
                double t0 = now();
                run_with_mate_slack(c, (uint32_t)r, lo, std::min<uint64_t>(hi_, 0x7FFFFFFFull), true);
                busy_run[k] += now() - t0;
                t0 = now();
                rp.collect(c, mine);
                busy_out[k] += now() - t0;
            }
        });
    }

    // ---- window (--overlap 0) ----
    void window(WindowPrinter& wp, WindowData& wd) {
        const uint64_t w = o.window;
        const std::vector<sbx_shard> sh = plan((uint32_t)w);
        const size_t n_ref = (size_t)ref_count(), S = wp.S(), cstride = std::max<size_t>(1, o.thresholds.size());
        wd.base.assign(n_ref + 1, 0); wd.n_full.assign(n_ref, 0);
        wd.extra_st.assign(n_ref, {}); wd.extra_cov.assign(n_ref, {});
        wd.has_cols.assign(n_ref, 0); wd.firstcol.assign(n_ref, ~0ULL); wd.lastcol.assign(n_ref, 0);
        uint64_t total = 0;
        for (size_t r = 0; r < n_ref; ++r) {
            wd.base[r] = total;
            wd.n_full[r] = ref_len(ctx0, (int)r) / w;
            total += wd.n_full[r];
        }
        wd.base[n_ref] = total;
        wd.st.assign((size_t)total * S, sbx_region_stats{0, 0});
        wd.cov.assign((size_t)total * S * cstride, 0);
        run_workers([&](size_t k, sbx_ctx* c) {
            WindowPrinter local{c, o, out, samples};       // its window_stats() on this device's run
            for (const sbx_shard& x : sh) {
                if (x.shard != k) continue;
                const uint32_t r = x.ref_id;
                const uint64_t len = (uint64_t)sbx_ref_length(c, (int)r);
                double t0 = now();
                const bool last = x.end >= len;
                run_with_mate_slack(c, r, x.beg, last ? kBaiEnd : x.end, false);
                busy_run[k] += now() - t0;
                t0 = now();
                uint64_t fc = 0, lc = 0;
                const bool any = first_column_in(c, r, x.beg, last ? kPrintToEnd : x.end, &fc);
                if (any && last) last_column_from(c, r, x.beg, &lc);
                const uint64_t k0 = x.beg / w, k1 = last ? len / w : x.end / w;            // only full windows are printed
                const uint64_t CH = 1u << 18;
                std::vector<sbx_region_stats> st;
                std::vector<uint32_t> cv2;
                for (uint64_t a = k0; a < k1; a += CH) {      // (full, disjoint windows: window_stats() asks the engine, rows max(1, n_thr) wide)
                    const uint64_t b = std::min(k1, a + CH);
                    local.window_stats((int)r, a, b, st, cv2);
                    std::copy(st.begin(), st.end(), wd.st.begin() + (size_t)(wd.base[r] + a) * S);
                    std::copy(cv2.begin(), cv2.end(), wd.cov.begin() + (size_t)(wd.base[r] + a) * S * cstride);
                }
                std::vector<sbx_region_stats> xs;
                std::vector<uint32_t> xc;
                if (any && last) {
                    // behind the contig's end: the windows that alignments hanging over it finish (depth.d:1057-1071 sees columns, not
                    // lengths), and the one the ring still holds when the contig ends
                    const uint64_t nw = std::max<uint64_t>(len >= w ? (len - w) / w + 1 : 0, lc >= w ? (lc - w) / w + 1 : 0);
                    const uint64_t nf = len / w;
                    local.window_stats((int)r, nf, nw + 1, xs, xc);
                }
                busy_out[k] += now() - t0;
                std::lock_guard<std::mutex> lk(sync.mu);
                if (any) {
                    wd.has_cols[r] = 1;
                    wd.firstcol[r] = std::min(wd.firstcol[r], fc);
                    if (last) { wd.lastcol[r] = lc; wd.extra_st[r] = std::move(xs); wd.extra_cov[r] = std::move(xc); }
                }
            }
        });
        // a contig whose LAST slice holds no column but an earlier one does: its last column lies in an earlier slice, within the contig --
        // every window that can be finished is a full one; the printer asks for the last column only to find windows behind the end
        for (size_t r = 0; r < n_ref; ++r)
            if (wd.has_cols[r] && wd.extra_st[r].empty()) {
                wd.lastcol[r] = 0;
                wd.extra_st[r].assign(S, sbx_region_stats{0, 0});
                wd.extra_cov[r].assign(S * cstride, 0);
            }
    }
    void report(double t_start) {
        std::string a;
        for (size_t k = 0; k < devices.size(); ++k) {
            char b[96];
            snprintf(b, sizeof b, " [device %d: run %.3f s, output %.3f s]", devices[k], busy_run[k], busy_out[k]);
            a += b;
        }
        fprintf(stderr, "[sbx-depth] sharded over %zu contexts:%s, total %.3f s since main\n", devices.size(), a.c_str(), now() - t_start);
    }
};

}  // namespace sbx
