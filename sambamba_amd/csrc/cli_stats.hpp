// cli_stats.hpp -- `depth region` and `depth window` of sbx-depth: the BED-style rows (print_region_row), where the first and
// last pileup columns of a run lie, and the reference's PerWindowPrinter / PerBedRegionPrinter fed from the device's statistics.
#pragma once
#include <cmath>

#include "cli_common.hpp"

namespace sbx {

inline std::string fmt_g(float f) {  // D's write(float) == %g with 6 significant digits (depth.d:859-864)
    char b[64];
    snprintf(b, sizeof b, "%g", (double)f);
    return b;
}

inline void print_bed_header(Out& out, const Options& o, size_t n_before) {  // depth.d:643-659
    static const char* def[] = {"chrom", "chromStart", "chromEnd"};
    std::string h = "# ";
    for (size_t i = 0; i < std::min<size_t>(3, n_before); ++i) h += std::string(def[i]) + "\t";
    for (size_t k = 3; k < n_before; ++k) h += "F" + std::to_string(k) + "\t";
    h += "readCount\tmeanCoverage";
    for (auto t : o.thresholds) h += "\tpercentage" + std::to_string(t);
    if (!o.combined) h += "\tsampleName";
    if (o.annotate) h += "\tmeanCovWithinBounds";
    h += "\n";
    out.put(h);
}

// printRegionStats (depth.d:847-876)
inline void print_region_row(Out& out, const Options& o, const std::string& prefix, uint32_t length, const sbx_region_stats& st,
                      const uint32_t* cov, const std::string& sample) {
    float mean_cov = (float)st.n_bases / (float)length;
    bool ok = (double)mean_cov >= o.min_cov && (double)mean_cov <= o.max_cov;
    if (!ok && !o.annotate) return;
    std::string row = prefix;
    row += std::to_string(st.n_reads) + "\t" + fmt_g(mean_cov);
    for (size_t j = 0; j < o.thresholds.size(); ++j) {
        float pct = (float)cov[j] * 100 / (float)length;
        if (o.thresholds[j] == 0) pct = 100.0f;
        row += "\t" + fmt_g(pct);
    }
    if (!o.combined) row += "\t" + sample;
    if (o.annotate) row += ok ? "\ty" : "\tn";
    row += "\n";
    out.put(row);
}


// first / last pileup column of the resident run inside [b, e) of contig r: `covered` alone is fetched, 64 Ki positions at a time
inline bool first_column_between(sbx_ctx* c, uint32_t r, uint64_t b, uint64_t e, uint64_t* pos_out) {
    std::vector<uint8_t> cov;
    for (uint64_t p = b; p < e; p += 65536) {
        const uint64_t q = std::min(e, p + 65536);
        cov.resize((size_t)(q - p));
        check(c, sbx_depth_base_tile(c, r, (uint32_t)p, (uint32_t)q, nullptr, cov.data()));
        for (uint64_t x = p; x < q; ++x)
            if (cov[(size_t)(x - p)]) { *pos_out = x; return true; }
    }
    return false;
}
inline bool last_column_between(sbx_ctx* c, uint32_t r, uint64_t b, uint64_t e, uint64_t* pos_out) {
    std::vector<uint8_t> cov;
    for (uint64_t q = e; q > b;) {
        const uint64_t p = q > b + 65536 ? q - 65536 : b;
        cov.resize((size_t)(q - p));
        check(c, sbx_depth_base_tile(c, r, (uint32_t)p, (uint32_t)q, nullptr, cov.data()));
        for (uint64_t x = q; x > p; --x)
            if (cov[(size_t)(x - 1 - p)]) { *pos_out = x - 1; return true; }
        q = p;
    }
    return false;
}
// first / last pileup column of the resident run inside [beg, end) of contig r (a slice of a sharded job)
inline bool first_column_in(sbx_ctx* c, uint32_t r, uint64_t beg, uint64_t end, uint64_t* pos_out) {
    bool found = false;
    for_each_active_range(c, r, beg, end, [&](uint64_t b, uint64_t e) { return !(found = first_column_between(c, r, b, e, pos_out)); });
    return found;
}
inline bool last_column_from(sbx_ctx* c, uint32_t r, uint64_t beg, uint64_t* pos_out) {
    std::vector<std::pair<uint64_t, uint64_t>> runs;
    for_each_active_range(c, r, beg, kNoEnd, [&](uint64_t b, uint64_t e) { runs.push_back({b, e}); });
    for (size_t i = runs.size(); i-- > 0;)
        if (last_column_between(c, r, runs[i].first, runs[i].second, pos_out)) return true;
    return false;
}
// What a job sharded over several devices collected for the window printer (run_sharded): the statistics of every full window,
// of the windows behind a contig's end that alignments hanging over it finish or leave unfinished, the first column of the run
// and the last column of every contig -- everything PerWindowPrinter's rules below are stated in.
struct WindowData {
    std::vector<uint64_t> base, n_full;                   // per contig: index of its window 0 in st / cov, number of full windows
    std::vector<sbx_region_stats> st;                     // [window][S]
    std::vector<uint32_t> cov;                            // [window][S][max(1, n_thr)]
    std::vector<std::vector<sbx_region_stats>> extra_st;  // per contig: windows n_full ..
    std::vector<std::vector<uint32_t>> extra_cov;
    std::vector<char> has_cols;
    std::vector<uint64_t> firstcol, lastcol;
};

// PerWindowPrinter (depth.d:933-1077), fed one batch of contigs at a time.  Windows k = [k*step, k*step + w),
// step = w - overlap, live in a ring of n = ceil(w / step) slots in the reference; what it prints is, per window:
//   * n_reads / n_bases of the window as a region -- except in the FIRST ring of the run (windows 1 .. n-1 of contig 0
//     when the first pileup column lies on it): is_first_occurrence starts out false there (depth.d:1031-1032), so only
//     reads starting inside the window are counted;
//   * coverage thresholds over the columns in [cs, k*step + w), cs = (k - n)*step + w for k >= n: every column updates
//     all n slots of the ring (depth.d:215-226), including a slot whose window has not begun when w is not a multiple
//     of the step;
//   * all k with k*step + w <= length for a contig with columns, length / step all-zero windows for a read-less contig;
//     nothing for windows finished before the first column of the run (the sample list does not exist yet);
//   * the first read-less contig AFTER the last contig with columns continues that contig's window coordinates and
//     shows the statistics its unfinished windows held: close() does not reset the ring (depth.d:1070-1076).
struct WindowPrinter {
    sbx_ctx* c;
    const Options& o;
    Out& out;
    const std::vector<std::string>& samples;
    bool have_first = false;     // the first pileup column of the whole run has been seen
    int fref = 0;
    uint64_t fpos = 0;
    int last_cols_ref = -1;      // the last contig with columns so far, the number of windows it printed,
    uint64_t last_nl = 0;
    std::vector<sbx_region_stats> stale_st;      // and what its n unfinished windows hold
    std::vector<uint32_t> stale_cov;
    std::vector<int> pending_empty;              // read-less contigs seen since
    const WindowData* data = nullptr;            // a sharded job: the statistics were collected slice by slice; `c` answers for the header only

    bool has_columns(int r) {
        if (data) return data->has_cols[(size_t)r] != 0;
        return has_active_range(c, (uint32_t)r);
    }
    // position of the first pileup column of the run (first admitted read) in contigs [r0, r1), or false if there is none
    bool first_column(int r0, int r1) {
        for (int r = r0; r < r1; ++r) {
            if (data ? !data->has_cols[(size_t)r] : !first_column_in(c, (uint32_t)r, 0, kNoEnd, &fpos)) continue;
            if (data) fpos = data->firstcol[(size_t)r];
            fref = r;
            return true;
        }
        return false;
    }
    void collected_stats(int r, uint64_t k0, uint64_t k1, std::vector<sbx_region_stats>& st, std::vector<uint32_t>& cov) {
        const uint32_t s_n = S();
        const size_t cstride = std::max<size_t>(1, o.thresholds.size());
        const uint64_t nf = data->n_full[(size_t)r];
        const auto& xs = data->extra_st[(size_t)r];
        const auto& xc = data->extra_cov[(size_t)r];
        for (uint64_t k = k0; k < k1; ++k) {
            const sbx_region_stats* ps = nullptr;
            const uint32_t* pc = nullptr;
            if (k < nf) { ps = &data->st[(size_t)(data->base[(size_t)r] + k) * s_n]; pc = &data->cov[(size_t)(data->base[(size_t)r] + k) * s_n * cstride]; }
            else if ((k - nf + 1) * s_n <= xs.size()) { ps = &xs[(size_t)(k - nf) * s_n]; pc = &xc[(size_t)(k - nf) * s_n * cstride]; }
            if (!ps) continue;
            std::copy(ps, ps + s_n, st.begin() + (size_t)(k - k0) * s_n);
            std::copy(pc, pc + s_n * cstride, cov.begin() + (size_t)(k - k0) * s_n * cstride);
        }
    }

    uint32_t S() const { return o.combined ? 1u : (uint32_t)samples.size(); }
    uint64_t step() const { return (uint64_t)o.window - (uint64_t)o.overlap; }
    uint64_t ring() const { return ((uint64_t)o.window + step() - 1) / step(); }

    // statistics of windows [k0, k1) of contig r (st: [k][S], cov: [k][S][n_thr])
    void window_stats(int r, uint64_t k0, uint64_t k1, std::vector<sbx_region_stats>& st, std::vector<uint32_t>& cov) {
        const uint32_t s_n = S();
        const size_t n_thr = o.thresholds.size(), cstride = std::max<size_t>(1, n_thr);
        const uint64_t w = o.window, st_ = step(), n = ring();
        st.assign((size_t)(k1 - k0) * s_n, sbx_region_stats{0, 0});
        cov.assign((size_t)(k1 - k0) * s_n * cstride, 0);
        if (k1 <= k0) return;
        if (data) { collected_stats(r, k0, k1, st, cov); return; }
        const uint64_t len = ref_len(c, r);
        if (o.overlap == 0 && k1 * w <= len) {      // full, disjoint windows: the engine's own window statistics
            check(c, sbx_depth_window_stats(c, (uint32_t)r, k0, k1 - k0, st.data(), cov.data()));
            return;
        }
        // the first ring of the run
        const uint64_t anom_from = (r == 0 && fref == 0) ? (fpos < w ? 0 : (fpos - w) / st_ + 1) : n;
        std::vector<sbx_region> reg, creg;
        std::vector<uint32_t> min_start;
        bool any_min = false, extended = false;
        for (uint64_t k = k0; k < k1; ++k) {
            reg.push_back({(uint32_t)r, (uint32_t)(k * st_), (uint32_t)(k * st_ + w)});
            const bool anom = k >= 1 && k >= anom_from && k < n;
            min_start.push_back(anom ? (uint32_t)(k * st_) : 0u);
            any_min |= anom;
            const uint64_t cs = k < n ? k * st_ : (k - n) * st_ + w;
            extended |= cs != k * st_;
            creg.push_back({(uint32_t)r, (uint32_t)cs, (uint32_t)(k * st_ + w)});
        }
        std::vector<uint8_t> seen(reg.size());
        std::vector<uint32_t> cov1(reg.size() * s_n * cstride);
        if (any_min && o.fix_mate)
            throw Fail{"--fix-mate-overlaps with --overlap > 0: the first pileup column lies in the first ring of windows of the first contig "
                       "(the reference counts only reads that start inside those windows, depth.d:1031-1032); not supported on the device path"};
        if (any_min) check(c, sbx_depth_region_stats_from(c, reg.data(), reg.size(), min_start.data(), st.data(), cov1.data(), seen.data()));
        else check(c, sbx_depth_region_stats(c, reg.data(), reg.size(), st.data(), cov1.data(), seen.data()));
        if (extended && n_thr) {
            std::vector<sbx_region_stats> st2(reg.size() * s_n);
            check(c, sbx_depth_region_stats(c, creg.data(), creg.size(), st2.data(), cov1.data(), seen.data()));
        }
        for (size_t i = 0; i < reg.size() * s_n; ++i)
            for (size_t t = 0; t < n_thr; ++t) cov[i * cstride + t] = cov1[i * n_thr + t];
    }
    void rows(const std::string& name, uint64_t start, const sbx_region_stats* st, const uint32_t* cov) {
        const std::string prefix = name + "\t" + std::to_string(start) + "\t" + std::to_string(start + o.window) + "\t";
        static const sbx_region_stats zero{0, 0};
        static const uint32_t zcov[kMaxCliThresholds] = {0};
        const size_t cstride = std::max<size_t>(1, o.thresholds.size());
        for (uint32_t s2 = 0; s2 < S(); ++s2)
            print_region_row(out, o, prefix, (uint32_t)o.window, st ? st[s2] : zero, cov ? cov + s2 * cstride : zcov, samples[s2]);
    }
    void zero_windows(int r) {       // printEmptyWindows (depth.d:1039-1044)
        const uint64_t cnt = ref_len(c, r) / step();
        const std::string name = sbx_ref_name(c, r);
        for (uint64_t k = 0; k < cnt; ++k) rows(name, k * step(), nullptr, nullptr);
    }
    // position of the last pileup column of contig r (it has one)
    uint64_t last_column(int r) {
        if (data) return data->lastcol[(size_t)r];
        uint64_t lb = 0, le = 0, pos = 0;      // (its last active range holds it)
        for_each_active_range(c, (uint32_t)r, 0, kNoEnd, [&](uint64_t b, uint64_t e) { lb = b; le = e; });
        last_column_between(c, (uint32_t)r, lb, le, &pos);
        return pos;
    }
    void contig(int r) {
        const uint64_t len = ref_len(c, r), w = o.window;
        // windows are finished as the columns advance (push) and then up to the contig's length (close / contig change):
        // alignments hanging over the end of the contig can finish windows that end beyond it
        const uint64_t lastcol = last_column(r);
        const uint64_t nw = std::max<uint64_t>(len >= w ? (len - w) / step() + 1 : 0, lastcol >= w ? (lastcol - w) / step() + 1 : 0);
        const std::string name = sbx_ref_name(c, r);
        const size_t cstride = std::max<size_t>(1, o.thresholds.size());
        std::vector<sbx_region_stats> st;
        std::vector<uint32_t> cov;
        const uint64_t CH = 1u << 18;
        for (uint64_t k0 = 0; k0 < nw; k0 += CH) {
            const uint64_t k1 = std::min(nw, k0 + CH);
            window_stats(r, k0, k1, st, cov);
            for (uint64_t k = k0; k < k1; ++k) {
                if (r == fref && k * step() + w <= fpos) continue;       // finished before the first column of the run
                rows(name, k * step(), &st[(size_t)(k - k0) * S()], &cov[(size_t)(k - k0) * S() * cstride]);
            }
        }
        // what the ring still holds when this contig ends
        last_cols_ref = r;
        last_nl = nw;
        window_stats(r, nw, nw + ring(), stale_st, stale_cov);
    }
    void run_refs(int r0, int r1) {
        // --fix-mate-overlaps with overlapping windows: a window is the region [k step, k step + w) of the closed form (reduce.hip) as
        // long as (a) w is a multiple of the step -- otherwise a ring slot also collects per-COLUMN mate terms of the columns in front of
        // its window, which the closed form of a region does not know -- and (b) no window of the run's first ring is printed (window_stats
        // below: is_first_occurrence, depth.d:1031-1032, interacts with the mate status there).  Everything else is refused.
        if (o.overlap > 0 && o.fix_mate && o.window % step() != 0)
            throw Fail{"--fix-mate-overlaps with an --overlap whose step (window - overlap) does not divide the window is not supported on the device path"};
        if (!have_first) {
            if (!first_column(r0, r1)) return;   // no column yet: windows so far print nothing
            have_first = true;
        }
        for (int r = std::max(r0, fref); r < r1; ++r) {
            if (!has_columns(r)) { pending_empty.push_back(r); continue; }
            for (int e : pending_empty) zero_windows(e);      // read-less contigs between two with columns: push() resets first
            pending_empty.clear();
            contig(r);
        }
    }
    void finish() {
        if (!have_first) return;
        bool first = true;
        const size_t cstride = std::max<size_t>(1, o.thresholds.size());
        for (int e : pending_empty) {
            if (first && last_cols_ref >= 0) {
                const uint64_t cnt = ref_len(c, e) / step();
                const std::string name = sbx_ref_name(c, e);
                for (uint64_t i = 0; i < cnt; ++i) {
                    if (i < ring()) rows(name, (last_nl + i) * step(), &stale_st[(size_t)i * S()], &stale_cov[(size_t)i * S() * cstride]);
                    else rows(name, (last_nl + i) * step(), nullptr, nullptr);
                }
            } else zero_windows(e);
            first = false;
        }
    }
};

// PerBedRegionPrinter (depth.d:879-931): statistics are gathered batch by batch, rows are printed at the end
// in input order -- and not at all unless some column fell inside some region (the samples array is created
// lazily)
struct RegionPrinter {
    sbx_ctx* c;
    const Options& o;
    Out& out;
    const std::vector<std::string>& samples;
    const std::vector<sbx_region>& raw;
    const std::vector<std::string>& lines;
    std::vector<sbx_region_stats> st;
    std::vector<uint32_t> cov;
    std::vector<uint8_t> seen;

    uint32_t n_samples() const { return o.combined ? 1u : (uint32_t)samples.size(); }
    size_t stride() const { return std::max<size_t>(1, o.thresholds.size()); }
    void prepare() {
        const size_t S = n_samples(), n_thr = stride();
        if (st.empty()) { st.assign(raw.size() * S, sbx_region_stats{0, 0}); cov.assign(raw.size() * S * n_thr, 0); seen.assign(raw.size(), 0); }
    }
    void run_refs(int r0, int r1) {
        prepare();
        std::vector<size_t> ids;
        for (size_t i = 0; i < raw.size(); ++i)
            if ((int)raw[i].ref_id >= r0 && (int)raw[i].ref_id < r1) ids.push_back(i);
        collect(c, ids);
    }
    // statistics of the raw regions `ids` from the run resident in context cx (a sharded job: the device that owns them; the rows
    // of different devices are disjoint, prepare() has been called before the threads started)
    void collect(sbx_ctx* cx, const std::vector<size_t>& ids) {
        const size_t S = n_samples(), n_thr = stride();
        std::vector<sbx_region> sub;
        for (size_t i : ids) sub.push_back(raw[i]);
        if (sub.empty()) return;
        std::vector<sbx_region_stats> st2(sub.size() * S);
        std::vector<uint32_t> cov2(sub.size() * S * n_thr);
        std::vector<uint8_t> seen2(sub.size());
        check(cx, sbx_depth_region_stats(cx, sub.data(), sub.size(), st2.data(), cov2.data(), seen2.data()));
        const size_t nt = o.thresholds.size();
        for (size_t j = 0; j < ids.size(); ++j) {
            seen[ids[j]] = seen2[j];
            for (uint32_t s2 = 0; s2 < S; ++s2) {
                st[ids[j] * S + s2] = st2[j * S + s2];
                for (size_t t = 0; t < nt; ++t) cov[(ids[j] * S + s2) * n_thr + t] = cov2[(j * S + s2) * nt + t];
            }
        }
    }
    void finish() {
        const size_t S = n_samples(), n_thr = stride();
        bool any = false;
        for (auto v : seen) any |= v != 0;
        if (!any) return;
        for (size_t id = 0; id < raw.size(); ++id) {
            std::string l = lines[id];
            while (!l.empty() && isspace((unsigned char)l.back())) l.pop_back();   // stripRight (depth.d:904)
            l += "\t";
            for (uint32_t s2 = 0; s2 < S; ++s2)
                print_region_row(out, o, l, raw[id].end - raw[id].start, st[id * S + s2], &cov[(id * S + s2) * n_thr], samples[s2]);
        }
    }
};

}  // namespace sbx
