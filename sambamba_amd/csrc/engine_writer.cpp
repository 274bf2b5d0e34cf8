// engine_writer.cpp -- the write side and the passes over the record stream of one file: BGZF compression on the device
// (sbx_bgzf_compress, sbx_write_bam), and the index-mode passes in batches (for_each_record_batch, engine_stream.hpp) behind
// sbx_build_index and sbx_flagstat.  (sbx_sort_bam, which is both, lives in engine_sort.cpp.)
#include <algorithm>
#include <cstdlib>

#include "bai_parallel.hpp"
#include "bai_writer.hpp"
#include "bins.hpp"
#include "bins_core.hpp"
#include "deflate_core.hpp"
#include "engine_ctx.hpp"
#include "engine_stream.hpp"
#include "flagstat.hpp"

extern "C" {

int sbx_bgzf_compress(const uint8_t* in, size_t n, int level, int with_eof, int device, uint8_t* out, size_t cap, size_t* out_len,
                      char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if ((!in && n) || !out_len) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        require_device(device);
        size_t pos = 0;
        bgzf_compress_stream(in, n, level, [&](const uint8_t* p, size_t k) {
            if (pos + k > cap || !out) { pos += k; return; }
            memcpy(out + pos, p, k);
            pos += k;
        });
        if (with_eof) {
            if (out && pos + 28 <= cap) memcpy(out + pos, kEofBlock, 28);
            pos += 28;
        }
        *out_len = pos;
        if (pos > cap || !out) throw Error(SBX_ENOMEM, "output buffer too small for the BGZF stream");
    });
}

// ---- index-mode passes: the record stream of one file in batches (sbx_build_index, sbx_flagstat) ---------------------------------
extern "C++" {
namespace {
// the one body of sbx_build_index and sbx_index_bam; check_bins: `index -c` (K16a next to the pass, bins.hip)
int build_index_impl(const char* bam_path, const char* bai_path, bool check_bins, int device, char* err, size_t errlen) {
    return run_entry(err, errlen, [&] {
        if (!bam_path || !bai_path) throw Error(SBX_EINVAL, "null argument");
        Standalone ctx;
        try {
            ctx = open_record_pass(bam_path, device, nullptr, false);      // no filter: every record is described
        } catch (const Error& e) {
            throw Error(SBX_EIO, e.what());              // (whatever the open says: a BAM that cannot be indexed is an I/O failure here)
        }
        sbx_ctx* const c = ctx.get();
        // IndexBuilder is one pass over a stream of records (bai/indexing.d:262-316), and so is this: the file goes through the
        // device in batches of whole BGZF blocks (for_each_record_batch).
        const BlockTable& bt = c->blocks;
        const size_t nbk = bt.size();
        const uint64_t total = bt.out_off.back();
        const uint64_t file_end_coff = nbk ? bt.comp_off[nbk - 1] + bt.comp_len[nbk - 1] + 8 : 0;
        const uint64_t batch_u = index_batch_bytes();
        hipStream_t s = c->stream.get();
        const int n_ref = (int)c->hdr.refs.size();
        // What consumes the records of a batch: the device (bai_parallel.hpp -- one lane per record; only the run heads, about one
        // record in fifty, and a few per-reference arrays come back) or, for input that formulation calls irregular (unsorted reads:
        // the reference's error is worded by the serial builder; reads far beyond the end of their reference) and with
        // SBX_BAI_HOST=1, IndexBuilder's loop restated on the host (bai_writer.hpp) over descriptors copied back record by record.
        std::vector<uint8_t> bytes;
        uint32_t n_batches = 0;
        // -c: the count of placed records with a wrong bin and the number of the first, over the batches of a pass; the first one's
        // name and bins are fetched from the batch that holds it (the next batch overwrites U)
        DevBuf<unsigned long long> d_bin_acc(kBinCheckWords);
        unsigned long long bin_acc[kBinCheckWords] = {0, kBinCheckNone};
        std::string bin_complaint;
        auto check_batch = [&](uint64_t nrec, uint64_t rec_base, uint64_t u_end) {
            launch_check_bins(c->U(), c->d_desc.p, c->d_rec_ref.p, nrec, rec_base, u_end, d_bin_acc.p, s);
            SBX_HIP(hipMemcpyAsync(bin_acc, d_bin_acc.p, sizeof bin_acc, hipMemcpyDeviceToHost, s));
            SBX_HIP(hipStreamSynchronize(s));
            if (!bin_acc[kBinCheckBad] || !bin_complaint.empty()) return;
            const uint64_t i = bin_acc[kBinCheckFirst] - rec_base;
            if (i >= nrec) throw Error(SBX_EFORMAT, "internal error: the first record with a wrong bin is not in its batch");
            RecDesc d;
            SBX_HIP(hipMemcpy(&d, c->d_desc.p + i, sizeof d, hipMemcpyDeviceToHost));
            std::vector<uint8_t> rec(36 + (size_t)d.l_name + 4 * (size_t)d.n_cigar);
            SBX_HIP(hipMemcpy(rec.data(), c->U() + d.rec_off, rec.size(), hipMemcpyDeviceToHost));
            uint32_t want = 0;
            binc::expected_bin(rec.data(), binc::load32(rec.data()), &want);
            const char* name = (const char*)rec.data() + 36;
            bin_complaint = "Bin in read with name '" + std::string(name, strnlen(name, d.l_name)) + "' is set incorrectly (" +
                            std::to_string(binc::stored_bin(rec.data())) + " instead of expected " + std::to_string(want) + ")";
        };
        auto pass = [&](bool on_device) -> bool {
            if (check_bins) {
                bin_acc[kBinCheckBad] = 0; bin_acc[kBinCheckFirst] = kBinCheckNone;
                bin_complaint.clear();
                SBX_HIP(hipMemcpyAsync(d_bin_acc.p, bin_acc, sizeof bin_acc, hipMemcpyHostToDevice, s));
                SBX_HIP(hipStreamSynchronize(s));
            }
            uint64_t checked_base = 0;
            // serial consumer
            VoffCursor vc(bt.coffset.data(), bt.out_off.data(), nbk, file_end_coff);
            BaiBuilder bb(n_ref);
            BaiRecord held;                 // the last record of the batch before: it ends where the next batch starts
            bool have_held = false;
            DevBuf<uint16_t> d_bins;
            std::vector<RecDesc> desc;
            std::vector<int32_t> ref;
            std::vector<uint16_t> bins;
            // device consumer
            BaiHostResults R;
            DevBuf<uint64_t> d_coff, d_ustart, d_lin, d_meta;      // d_meta: meta_end | n_mapped | n_unmapped, n_ref + 1 each
            DevBuf<uint32_t> d_lin_off, d_lin_len;
            DevBuf<unsigned long long> d_scalars;
            DevBuf<BaiRun> d_runs;
            DevBuf<BaiCarry> d_carry(1);
            BaiCarry carry{-1, 0, 0, 0, 0};
            uint64_t rec_base = 0;
            if (on_device) {
                R.lin_off.assign((size_t)n_ref + 1, 0);
                for (int r = 0; r < n_ref; ++r) R.lin_off[(size_t)r + 1] = R.lin_off[(size_t)r] + bai_windows_for(c->hdr.refs[(size_t)r].length);
                d_coff.alloc(nbk + 1); d_ustart.alloc(nbk + 2);
                d_lin.alloc((size_t)R.lin_off[(size_t)n_ref] + 1); d_lin_off.alloc((size_t)n_ref + 2); d_lin_len.alloc((size_t)n_ref + 1);
                d_meta.alloc(3 * ((size_t)n_ref + 1)); d_scalars.alloc(kBaiScalars);
                if (nbk) SBX_HIP(hipMemcpyAsync(d_coff.p, bt.coffset.data(), nbk * 8, hipMemcpyHostToDevice, s));
                SBX_HIP(hipMemcpyAsync(d_ustart.p, bt.out_off.data(), (nbk + 1) * 8, hipMemcpyHostToDevice, s));
                SBX_HIP(hipMemcpyAsync(d_lin_off.p, R.lin_off.data(), ((size_t)n_ref + 1) * 4, hipMemcpyHostToDevice, s));
                SBX_HIP(hipMemsetAsync(d_lin.p, 0xFF, d_lin.bytes(), s));
                SBX_HIP(hipMemsetAsync(d_lin_len.p, 0, d_lin_len.bytes(), s));
                SBX_HIP(hipMemsetAsync(d_meta.p, 0, d_meta.bytes(), s));
                SBX_HIP(hipMemsetAsync(d_scalars.p, 0, d_scalars.bytes(), s));
                SBX_HIP(hipMemsetAsync(d_scalars.p + kBaiFirstVo, 0xFF, 8, s));
            }
            const bool whole = for_each_record_batch(c, batch_u, &n_batches, [&](uint64_t nrec, uint64_t base, uint64_t next) -> bool {
                if (check_bins) { check_batch(nrec, checked_base, next - base); checked_base += nrec; }
                if (on_device) {
                    const uint64_t cap = nrec / 4 + 4096;
                    d_runs.ensure((size_t)cap);
                    SBX_HIP(hipMemsetAsync(d_scalars.p + kBaiNumRuns, 0, 8, s));
                    BaiArgs a{};
                    a.U = c->U(); a.desc = c->d_desc.p; a.rec_ref = c->d_rec_ref.p; a.n = nrec; a.rec_base = rec_base;
                    a.u_base = base; a.u_next = next;
                    a.coff = d_coff.p; a.ustart = d_ustart.p; a.n_blocks = (uint32_t)nbk; a.file_end = file_end_coff;
                    a.carry = carry; a.n_ref = n_ref;
                    a.lin = d_lin.p; a.lin_off = d_lin_off.p; a.lin_len = d_lin_len.p;
                    a.meta_end = d_meta.p; a.n_mapped = d_meta.p + (n_ref + 1); a.n_unmapped = d_meta.p + 2 * ((size_t)n_ref + 1);
                    a.scalars = d_scalars.p; a.runs = d_runs.p; a.runs_cap = cap;
                    launch_bai_records(a, d_carry.p, s);
                    unsigned long long sc[kBaiScalars];
                    SBX_HIP(hipMemcpyAsync(sc, d_scalars.p, sizeof sc, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipMemcpyAsync(&carry, d_carry.p, sizeof carry, hipMemcpyDeviceToHost, s));
                    SBX_HIP(hipStreamSynchronize(s));
                    if (sc[kBaiIrregular] || sc[kBaiNumRuns] > cap) return false;
                    const size_t at = R.runs.size(), nr = (size_t)sc[kBaiNumRuns];
                    R.runs.resize(at + nr);
                    if (nr) SBX_HIP(hipMemcpy(R.runs.data() + at, d_runs.p, nr * sizeof(BaiRun), hipMemcpyDeviceToHost));
                    rec_base += nrec;
                } else {
                    d_bins.ensure((size_t)nrec + 1);
                    launch_gather_bins(c->U(), c->d_desc.p, nrec, d_bins.p, s);
                    desc.resize((size_t)nrec); ref.resize((size_t)nrec); bins.resize((size_t)nrec);
                    SBX_HIP(hipStreamSynchronize(s));
                    if (nrec) {
                        SBX_HIP(hipMemcpy(desc.data(), c->d_desc.p, (size_t)nrec * sizeof(RecDesc), hipMemcpyDeviceToHost));
                        SBX_HIP(hipMemcpy(ref.data(), c->d_rec_ref.p, (size_t)nrec * 4, hipMemcpyDeviceToHost));
                        SBX_HIP(hipMemcpy(bins.data(), d_bins.p, (size_t)nrec * 2, hipMemcpyDeviceToHost));
                    }
                    for (uint64_t i = 0; i < nrec; ++i) {
                        const uint64_t at = base + desc[(size_t)i].rec_off;
                        if (have_held) { held.end_vo = vc.behind(at); bb.put(held); }
                        held.ref_id = ref[(size_t)i];
                        held.position = desc[(size_t)i].pos;
                        held.end_position = desc[(size_t)i].end;
                        held.bin = bins[(size_t)i];
                        held.is_unmapped = (desc[(size_t)i].flag & 0x4) != 0;
                        held.start_vo = vc.of_byte(at);
                        have_held = true;
                    }
                }
                return true;
            });
            if (!whole) return false;
            if (on_device) {
                const size_t m = (size_t)n_ref + 1;
                R.lin.resize(d_lin.n); R.lin_len.resize(m); R.meta_end.resize(m); R.n_mapped.resize(m); R.n_unmapped.resize(m);
                unsigned long long sc[kBaiScalars];
                SBX_HIP(hipMemcpy(R.lin.data(), d_lin.p, d_lin.n * 8, hipMemcpyDeviceToHost));
                SBX_HIP(hipMemcpy(R.lin_len.data(), d_lin_len.p, m * 4, hipMemcpyDeviceToHost));
                SBX_HIP(hipMemcpy(R.meta_end.data(), d_meta.p, m * 8, hipMemcpyDeviceToHost));
                SBX_HIP(hipMemcpy(R.n_mapped.data(), d_meta.p + m, m * 8, hipMemcpyDeviceToHost));
                SBX_HIP(hipMemcpy(R.n_unmapped.data(), d_meta.p + 2 * m, m * 8, hipMemcpyDeviceToHost));
                SBX_HIP(hipMemcpy(sc, d_scalars.p, sizeof sc, hipMemcpyDeviceToHost));
                for (int k = 0; k < (int)kBaiScalars; ++k) R.scalars[k] = sc[k];
                R.last = carry;
                bytes = bai_assemble(n_ref, R);
            } else {
                if (have_held) { held.end_vo = vc.behind(total); bb.put(held); }
                bytes = bb.finish();
            }
            return true;
        };
        const bool host_only = getenv("SBX_BAI_HOST") != nullptr;
        bool on_device = !host_only;
        if (on_device && !pass(true)) on_device = false;
        if (!on_device) pass(false);
        // (an unsorted file has left through the serial builder's refusal by now, whichever fault comes first in the file)
        if (check_bins && bin_acc[kBinCheckBad])
            throw Error(SBX_EFORMAT, bin_complaint + "; " + std::to_string(bin_acc[kBinCheckBad]) +
                                         (bin_acc[kBinCheckBad] == 1 ? " record of the file has a wrong bin" : " records of the file have a wrong bin"));
        if (getenv("SBX_TIMING"))
            fprintf(stderr, "[sbx] build_index: %u batch(es) of <= %llu inflated bytes, records consumed %s\n", n_batches, (unsigned long long)batch_u,
                    on_device ? "on the device" : "by the serial builder on the host");
        OutputFile f(bai_path);
        f.write(bytes.data(), bytes.size());
        f.finish(false);
    });
}
}  // namespace
}  // extern "C++"

int sbx_build_index(const char* bam_path, const char* bai_path, int device, char* err, size_t errlen) {
    return build_index_impl(bam_path, bai_path, false, device, err, errlen);
}

int sbx_index_bam(const char* bam_path, const char* bai_path, int check_bins, int device, char* err, size_t errlen) {
    return build_index_impl(bam_path, bai_path, check_bins != 0, device, err, errlen);
}

// `sambamba flagstat` (computeFlagStatistics, flagstat.d:31-58): one pass like sbx_build_index's -- index mode, no filter, no sort
// order or index required -- with K8 (flagstat.hip) adding each batch's records to 26 device counters, read back once at the end.
// Every record of the chain is counted, also one that index mode calls bad (refID out of range, lengths that disagree with
// block_size) or one that starts beyond its contig: the reference reads nothing but the flags, mapq and the two reference ids.
int sbx_flagstat(const char* bam_path, int device, sbx_flagstat_counts* out, char* err, size_t errlen) {
    static_assert(sizeof(sbx_flagstat_counts) == 26 * sizeof(uint64_t), "sbx_flagstat_counts is the kernel's 26 counters");
    return run_entry(err, errlen, [&] {
        if (!bam_path || !out) throw Error(SBX_EINVAL, "null argument");
        const double w0 = wall_now();
        Standalone c = open_record_pass(bam_path, device, nullptr, false);      // no filter: every record is described
        hipStream_t s = c->stream.get();
        DevBuf<unsigned long long> d_counts(26);
        SBX_HIP(hipMemsetAsync(d_counts.p, 0, d_counts.bytes(), s));
        const bool timing = getenv("SBX_TIMING") != nullptr;
        const double w1 = wall_now();
        EventTimer t_k;
        double ms_inflate = 0, ms_index = 0, ms_k8 = 0;
        uint64_t n_records = 0;
        uint32_t n_batches = 0;
        for_each_record_batch(c.get(), index_batch_bytes(), &n_batches, [&](uint64_t nrec, uint64_t, uint64_t) -> bool {
            t_k.start(s);
            launch_flagstat(c->U(), c->d_desc.p, c->d_rec_ref.p, nrec, d_counts.p, s);
            t_k.stop(s);
            // (the next batch's K2 overwrites these descriptors, and may reallocate them, from the host side: K8 ends first)
            SBX_HIP(hipStreamSynchronize(s));
            if (timing) { ms_inflate += c->stats.ms_inflate; ms_index += c->stats.ms_index; ms_k8 += t_k.ms(); }
            n_records += nrec;
            return true;
        });
        sbx_flagstat_counts r{};
        SBX_HIP(hipMemcpyAsync(&r, d_counts.p, sizeof r, hipMemcpyDeviceToHost, s));
        SBX_HIP(hipStreamSynchronize(s));
        if (r.reads[0] + r.reads[1] != n_records)
            throw Error(SBX_EFORMAT, "internal error: flagstat counted " + std::to_string(r.reads[0] + r.reads[1]) + " of " +
                                         std::to_string(n_records) + " records");
        *out = r;
        if (timing)
            fprintf(stderr, "[sbx] flagstat: %llu records in %u batch(es): inflate %.2f ms, record index %.2f ms, flagstat kernel %.3f ms; "
                            "open %.1f ms, pass %.1f ms (wall)\n", (unsigned long long)n_records, n_batches, ms_inflate, ms_index, ms_k8,
                    (w1 - w0) * 1e3, (wall_now() - w1) * 1e3);
    });
}

extern "C++" {
namespace {
// percent / percentStr of flagstat.d:66-72: to!float(a) / b is single precision, `* 100.0` double, returned as float
void percent_str(uint64_t a, uint64_t b, char* buf, size_t n) {
    if (b == 0) { snprintf(buf, n, "N/A"); return; }
    const float p = (float)((double)((float)a / (float)b) * 100.0);
    snprintf(buf, n, "%.2f%%", (double)p);
}
}  // namespace
}  // extern "C++"

int sbx_format_flagstat(const sbx_flagstat_counts* f, int tabular, char* buf, size_t cap, size_t* len) {
    if (!f) return SBX_EINVAL;
    std::string out;
    char line[256], p0[32], p1[32];
    auto param = [&](const char* what, const uint64_t* v) {
        if (tabular) snprintf(line, sizeof line, "%s,%llu,%llu\n", what, (unsigned long long)v[0], (unsigned long long)v[1]);
        else snprintf(line, sizeof line, "%llu + %llu %s\n", (unsigned long long)v[0], (unsigned long long)v[1], what);
        out += line;
    };
    auto with_pct = [&](const char* what, const uint64_t* v, const uint64_t* total) {
        percent_str(v[0], total[0], p0, sizeof p0);
        percent_str(v[1], total[1], p1, sizeof p1);
        if (tabular) snprintf(line, sizeof line, "%s,%llu:%s,%llu:%s\n", what, (unsigned long long)v[0], p0, (unsigned long long)v[1], p1);
        else snprintf(line, sizeof line, "%llu + %llu %s (%s:%s)\n", (unsigned long long)v[0], (unsigned long long)v[1], what, p0, p1);
        out += line;
    };
    // flagstat.d:131-143
    param("in total (QC-passed reads + QC-failed reads)", f->reads);
    param("secondary", f->secondary);
    param("supplementary", f->supplementary);
    param("duplicates", f->dup);
    with_pct("mapped", f->mapped, f->reads);
    param("paired in sequencing", f->pair_all);
    param("read1", f->first);
    param("read2", f->second);
    with_pct("properly paired", f->pair_good, f->pair_all);
    param("with itself and mate mapped", f->pair_map);
    with_pct("singletons", f->single, f->pair_all);
    param("with mate mapped to a different chr", f->diff_chr);
    param("with mate mapped to a different chr (mapQ>=5)", f->diff_high);
    return copy_to_caller(out, buf, cap, len);
}

int sbx_write_bam(const char* path, const uint8_t* stream, size_t n, int level, int with_index, int device, char* err, size_t errlen) {
    const int rc = run_entry(err, errlen, [&] {
        if (!path || (!stream && n)) throw Error(SBX_EINVAL, "null argument");
        check_level(level);
        require_device(device);
        OutputFile f(path);
        bgzf_compress_stream(stream, n, level, [&](const uint8_t* p, size_t k) { f.write(p, k); });
        f.finish(true);
    });
    if (rc != SBX_OK || !with_index) return rc;
    return sbx_build_index(path, (std::string(path) + ".bai").c_str(), device, err, errlen);
}

}  // extern "C"
