// cli_base.hpp -- `depth base` of sbx-depth: the text of a stretch of a contig streamed from the device (stream_base_rows, the one
// routine behind the pipelined slices and the slices of a sharded job) and BasePrinter, the reference's PerBasePrinter.
#pragma once
#include <cstring>

#include "cli_common.hpp"

namespace sbx {

inline void print_base_header(Out& out, const Options& o) {
    out.put(std::string("REF\tPOS\tCOV\tA\tC\tG\tT\tDEL\tREFSKIP") + (o.combined ? "" : "\tSAMPLE") + (o.annotate ? "\tFLAG" : "") + "\n");
}

inline int write_to_file(void* u, const char* d, size_t n) { return fwrite(d, 1, n, (FILE*)u) == n ? 0 : 1; }

// the rows of [beg, end) of contig r from the run resident in context c, formatted on the device, through `write`
inline void stream_base_rows(sbx_ctx* c, const Options& o, uint32_t r, uint64_t beg, uint64_t end, sbx_write_fn write, void* user) {
    for_each_active_range(c, r, beg, end, [&](uint64_t b, uint64_t e) {
        check(c, sbx_stream_base_rows(c, r, (uint32_t)b, (uint32_t)e, o.min_cov, o.max_cov, o.annotate ? 1 : 0, write, user));
    });
}

// ---------------------------------------------------------------------------------------------
// depth base: PerBasePrinter (depth.d:402-607) driven from the device's dense counter tiles.
// A "column" exists at every position spanned by >= 1 admitted read (covered[] from the device).
// ---------------------------------------------------------------------------------------------
class BasePrinter {
public:
    BasePrinter(sbx_ctx* c, const Options& o, Out& out, const std::vector<std::string>& samples)
        : c_(c), o_(o), out_(out), samples_(samples) {
        sbx_header_info hi;
        sbx_header(c, &hi);
        n_ref_ = hi.n_ref;
        S_ = o.combined ? 1u : (uint32_t)samples.size();
    }
    void set_bed(const std::vector<sbx_region>& bed) { bed_ = bed; raw_ = bed; bed_provided_ = true; cur_head_ = 0; raw_head_ = 0; }
    // Device-formatted output (K6, sbx_format_base_rows): without -L the text is a pure function of the
    // position -- a column's rows, or with min_cov == 0 all-zero rows for every position of every contig
    // (what push/close/writeEmptyColumns add up to) -- and with -L and min_cov > 0 it is the same restricted
    // to the merged regions (outputRequired, depth.d:558-565).  -L with min_cov == 0 keeps the stateful
    // host emulation below (raw BED consumption quirks of writeEmptyColumns).
    bool device_format_applies() const {
        if (getenv("SBX_HOST_FORMAT")) return false;
        if (o_.min_cov < 0) return false;
        return !bed_provided_ || o_.min_cov > 0;
    }
    void run_device(int r0, int r1) {
        // the library formats on the device and hands the text over piece by piece (pinned buffers, the next piece is
        // formatted and copied while this one is written)
        auto range = [&](uint32_t r, uint64_t b, uint64_t e) {
            out_.flush();
            check(c_, sbx_stream_base_rows(c_, r, (uint32_t)b, (uint32_t)e, o_.min_cov, o_.max_cov, o_.annotate ? 1 : 0, write_to_file, out_.fp));
        };
        if (bed_provided_) {      // merged, sorted regions
            for (auto& g : bed_)
                if ((int)g.ref_id >= r0 && (int)g.ref_id < r1) range(g.ref_id, g.start, g.end);
            return;
        }
        for (int r = r0; r < r1; ++r) {
            const uint64_t len = (uint64_t)sbx_ref_length(c_, r);
            if (o_.min_cov == 0) {
                // Every position of a contig with pileup columns has rows.  A contig WITHOUT columns is zero-filled
                // only before the first and after the last contig that has some: push() fills from the previous
                // column's contig straight to the current one and skips what lies between (depth.d:574-583), close()
                // fills everything after the last column (depth.d:593-606).
                if (!has_active_range(c_, (uint32_t)r)) {
                    if (!seen_columns_) range((uint32_t)r, 0, len);
                    else pending_empty_.push_back(r);
                    continue;
                }
                seen_columns_ = true;
                pending_empty_.clear();
                range((uint32_t)r, 0, len);
            }
            // otherwise only stretches with admitted reads can have rows
            for_each_active_range(c_, (uint32_t)r, o_.min_cov == 0 ? len : 0, kNoEnd, [&](uint64_t b, uint64_t e) {
                if (o_.min_cov == 0) host_columns(r, b, e);       // alignments hanging over the contig end: columns only
                else range((uint32_t)r, b, e);
            });
        }
    }
    // rows of [beg, end) of contig r from context `c` (a slice of the pipelined run: min_cov > 0, no -L)
    void run_slice(sbx_ctx* c, uint32_t r, uint64_t beg, uint64_t end) {
        out_.flush();
        stream_base_rows(c, o_, r, beg, end, write_to_file, out_.fp);
    }
    void run_device_empty(int r) {
        std::vector<char> text;
        const uint64_t len = (uint64_t)sbx_ref_length(c_, r), CH = 8u << 20;
        for (uint64_t p = 0; p < len; p += CH) {
            const uint64_t q = std::min(len, p + CH);
            size_t need = 0;
            text.resize((size_t)(q - p) * 40 * S_ + 64);
            int rc = sbx_format_base_rows(c_, (uint32_t)r, (uint32_t)p, (uint32_t)q, o_.min_cov, o_.max_cov, o_.annotate ? 1 : 0,
                                          text.data(), text.size(), &need);
            if (rc == SBX_ENOMEM && need > text.size()) {
                text.resize(need);
                rc = sbx_format_base_rows(c_, (uint32_t)r, (uint32_t)p, (uint32_t)q, o_.min_cov, o_.max_cov, o_.annotate ? 1 : 0,
                                          text.data(), text.size(), &need);
            }
            check(c_, rc);
            out_.flush();
            fwrite(text.data(), 1, need, out_.fp);
        }
    }
    // fn(x, counters) for every pileup column in [b, e) of contig r; the tiles are fetched 1 Mi positions at a time
    template <class F> void for_each_column(int r, uint64_t b, uint64_t e, F&& fn) {
        std::vector<uint32_t> cnt;
        std::vector<uint8_t> cov;
        for (uint64_t p = b, CH = 1u << 20; p < e; p += CH) {
            const uint64_t q = std::min(e, p + CH);
            cnt.resize((size_t)(q - p) * S_ * SBX_NCOUNTERS);
            cov.resize((size_t)(q - p));
            check(c_, sbx_depth_base_tile(c_, (uint32_t)r, (uint32_t)p, (uint32_t)q, cnt.data(), cov.data()));
            for (uint64_t x = p; x < q; ++x)
                if (cov[(size_t)(x - p)]) fn((int64_t)x, &cnt[(size_t)(x - p) * S_ * SBX_NCOUNTERS]);
        }
    }
    void host_columns(int r, uint64_t b, uint64_t e) {
        for_each_column(r, b, e, [&](int64_t x, const uint32_t* v) { write_column(r, x, v); });
        out_.flush();
    }
    // rows of contigs [r0, r1) (the batch the device has just processed); finish() after the last batch
    void run_refs(int r0, int r1) {
        if (device_format_applies()) { run_device(r0, r1); return; }
        for (int r = r0; r < r1; ++r)
            for_each_active_range(c_, (uint32_t)r, 0, kNoEnd, [&](uint64_t b, uint64_t e) {
                for_each_column(r, b, e, [&](int64_t x, const uint32_t* v) { push(r, x, v); });
            });
    }
    void finish() {
        if (!device_format_applies()) { close(); return; }
        if (o_.min_cov == 0 && !bed_provided_)       // contigs without columns after the last one that had some
            for (int r : pending_empty_) run_device_empty(r);
    }

private:
    sbx_ctx* c_;
    const Options& o_;
    Out& out_;
    const std::vector<std::string>& samples_;
    int n_ref_ = 0;
    uint32_t S_ = 1;
    bool bed_provided_ = false;
    std::vector<sbx_region> bed_;   // NonOverlappingRegionStatsCollector view (depth.d:171-198)
    size_t cur_head_ = 0;
    std::vector<sbx_region> raw_;   // raw_bed, consumed by writeEmptyColumns (depth.d:464-486)
    size_t raw_head_ = 0;
    int prev_ref_ = -2;
    int64_t prev_pos_ = 0;
    std::vector<std::string> tails_;
    bool seen_columns_ = false;            // device-formatted -c 0 output: has any contig so far had a pileup column?
    std::vector<int> pending_empty_;       // ... contigs without columns seen since the last one that had some

    static bool fully_left_of(const sbx_region& g, uint32_t ref, uint32_t pos) { return g.ref_id < ref || (g.ref_id == ref && g.end <= pos); }
    static bool overlaps(const sbx_region& g, uint32_t ref, uint32_t pos) { return g.ref_id == ref && g.start <= pos && pos < g.end; }

    bool output_required(int ref, int64_t pos) {  // depth.d:558-565
        if (!bed_provided_) return true;
        while (cur_head_ < bed_.size() && fully_left_of(bed_[cur_head_], (uint32_t)ref, (uint32_t)pos)) ++cur_head_;
        return cur_head_ < bed_.size() && overlaps(bed_[cur_head_], (uint32_t)ref, (uint32_t)pos);
    }
    void init_tails() {  // depth.d:436-450
        if (!tails_.empty()) return;
        if (o_.combined) {
            tails_.push_back("\t0\t0\t0\t0\t0\t0\t0");
            if (o_.annotate) tails_[0] += (o_.min_cov > 0 ? "\tn" : "\ty");
        } else {
            for (auto& s : samples_) {
                tails_.push_back("\t0\t0\t0\t0\t0\t0\t0\t" + s);
                if (o_.annotate) tails_.back() += (o_.min_cov > 0 ? "\tn" : "\ty");
            }
        }
    }
    void emit_empty(const char* ref_name, size_t ref_len, long from, long to) {
        char num[24];
        for (long pos = from; pos < to; ++pos) {
            char* e = num + sizeof num;
            char* s = u64toa((uint64_t)pos, e);
            for (auto& t : tails_) {
                out_.put(ref_name, ref_len);
                out_.put("\t", 1);
                out_.put(s, (size_t)(e - s));
                out_.put(t);
                out_.put("\n", 1);
            }
        }
    }
    void write_empty(long ref_id, long start, long end) {  // depth.d:452-487
        if (o_.min_cov > 0 && !o_.annotate) return;
        const char* name = sbx_ref_name(c_, (int)ref_id);
        size_t nl = strlen(name);
        init_tails();
        if (!bed_provided_) { emit_empty(name, nl, start, end); return; }
        if (raw_head_ >= raw_.size() || raw_[raw_head_].ref_id > (uint32_t)ref_id) return;
        while (raw_head_ < raw_.size() && raw_[raw_head_].ref_id < (uint32_t)ref_id) ++raw_head_;
        while (raw_head_ < raw_.size() && raw_[raw_head_].ref_id == (uint32_t)ref_id) {
            sbx_region& f = raw_[raw_head_];
            if (fully_left_of(f, (uint32_t)ref_id, (uint32_t)start)) { ++raw_head_; continue; }
            long from = std::max<long>(start, f.start), to = std::min<long>(end, f.end);
            if (from >= to) break;
            emit_empty(name, nl, from, to);
            f.start = (uint32_t)to;
            if (f.start >= f.end) ++raw_head_;
        }
        bed_.assign(raw_.begin() + (long)raw_head_, raw_.end());   // collector rebuilt from what is left (depth.d:485)
        cur_head_ = 0;
    }
    void write_column(int ref, int64_t pos, const uint32_t* cnt) {  // depth.d:534-555
        const char* name = sbx_ref_name(c_, ref);
        size_t nl = strlen(name);
        char num[24];
        for (uint32_t s = 0; s < S_; ++s) {
            const uint32_t* v = cnt + (size_t)s * SBX_NCOUNTERS;
            uint64_t total = (uint64_t)v[0] + v[1] + v[2] + v[3] + v[4] + v[5] + v[6];
            bool ok = (double)total >= o_.min_cov && (double)total <= o_.max_cov;
            if (!ok && !o_.annotate) return;  // return, not continue (depth.d:540-541)
            out_.put(name, nl);
            auto num_field = [&](uint64_t x) {
                char* e = num + sizeof num;
                char* b = u64toa(x, e);
                out_.put("\t", 1);
                out_.put(b, (size_t)(e - b));
            };
            num_field((uint64_t)pos);
            num_field(total);
            num_field(v[0]); num_field(v[1]); num_field(v[2]); num_field(v[3]);
            num_field(v[5]); num_field(v[6]);
            if (!o_.combined) { out_.put("\t", 1); out_.put(samples_[s]); }
            if (o_.annotate) out_.put(ok ? "\ty" : "\tn", 2);
            out_.put("\n", 1);
        }
    }
    void push(int ref, int64_t pos, const uint32_t* cnt) {  // depth.d:567-591
        if (o_.min_cov > 0) {
            if (output_required(ref, pos)) write_column(ref, pos, cnt);
            return;
        }
        if (prev_ref_ == -2) {
            for (int id = 0; id < ref; ++id) write_empty(id, 0, (long)sbx_ref_length(c_, id));
            write_empty(ref, 0, (long)pos);
        } else if (prev_ref_ != ref) {
            write_empty(prev_ref_, (long)prev_pos_ + 1, (long)sbx_ref_length(c_, prev_ref_));
            write_empty(ref, 0, (long)pos);
        } else if (prev_pos_ != pos - 1) {
            write_empty(ref, (long)prev_pos_ + 1, (long)pos);
        }
        prev_ref_ = ref;
        prev_pos_ = pos;
        if (output_required(ref, pos)) write_column(ref, pos, cnt);
    }
    void close() {  // depth.d:593-606
        if (!(o_.min_cov == 0)) return;
        if (prev_ref_ == -2) {
            for (int id = 0; id < n_ref_; ++id) write_empty(id, 0, (long)sbx_ref_length(c_, id));
        } else {
            write_empty(prev_ref_, (long)prev_pos_ + 1, (long)sbx_ref_length(c_, prev_ref_));
            for (int id = prev_ref_ + 1; id < n_ref_; ++id) write_empty(id, 0, (long)sbx_ref_length(c_, id));
        }
    }
};

}  // namespace sbx
