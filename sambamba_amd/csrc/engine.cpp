// engine.cpp -- the C ABI of libsbx_depth.so (include/sbx_depth.h): device bring-up, opening and closing a context, the header,
// the filter, parameters and regions, and the small queries about the last run.  The device pipeline
//   compressed BGZF blocks in HBM -> K1 inflate -> K2 record index -> K3 decode+accumulate -> counters in HBM
// lives next to it, one concern per file: engine_worklist.cpp (BAI -> work list -> bytes on the device), engine_run.cpp (the pass),
// engine_stats.cpp (counters, region and window statistics), engine_text.cpp (`depth base` text) and engine_writer.cpp (BGZF / BAM /
// BAI output, flagstat); engine_ctx.hpp holds the context they share.
// Host code is orchestration only; every byte of BGZF payload, every record and every counter is produced on the device.  There is
// no CPU fallback: without a HIP device the compute entry points fail with SBX_ENODEVICE.
#include <cstdlib>
#include <memory>
#include <thread>

#include "engine_ctx.hpp"

namespace sbx {

void require_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        throw Error(SBX_ENODEVICE, std::string("no HIP device available (libsbx_depth has no CPU fallback): ") +
                                       (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0) {
        const char* lr = getenv("LOCAL_RANK");
        device = lr ? atoi(lr) % n : 0;
    }
    if (device >= n) throw Error(SBX_ENODEVICE, "HIP device ordinal " + std::to_string(device) + " out of range");
    SBX_HIP(hipSetDevice(device));
}

thread_local int t_open_code = SBX_OK;

}  // namespace sbx

namespace {
void default_filter(sbx_filter* f) {
    FilterCompiler fc("mapping_quality > 0 and not duplicate and not failed_quality_control", f);  // depth.d:1159
    fc.compile();
}
}  // namespace

extern "C" {

size_t sbx_abi_sizeof(const char* name) {
    if (!name) return 0;
    const std::string n = name;
    if (n == "sbx_region") return sizeof(sbx_region);
    if (n == "sbx_region_stats") return sizeof(sbx_region_stats);
    if (n == "sbx_header_info") return sizeof(sbx_header_info);
    if (n == "sbx_regex_state") return sizeof(sbx_regex_state);
    if (n == "sbx_regex") return sizeof(sbx_regex);
    if (n == "sbx_filter_op") return sizeof(sbx_filter_op);
    if (n == "sbx_filter") return sizeof(sbx_filter);
    if (n == "sbx_batch") return sizeof(sbx_batch);
    if (n == "sbx_run_stats") return sizeof(sbx_run_stats);
    if (n == "sbx_shard") return sizeof(sbx_shard);
    if (n == "sbx_flagstat_counts") return sizeof(sbx_flagstat_counts);
    if (n == "sbx_sort_stats") return sizeof(sbx_sort_stats);
    if (n == "sbx_markdup_stats") return sizeof(sbx_markdup_stats);
    if (n == "sbx_markdup_stream_stats") return sizeof(sbx_markdup_stream_stats);
    if (n == "sbx_merge_stats") return sizeof(sbx_merge_stats);
    if (n == "sbx_merge_window_stats") return sizeof(sbx_merge_window_stats);
    if (n == "sbx_view_opts") return sizeof(sbx_view_opts);
    if (n == "sbx_view_stats") return sizeof(sbx_view_stats);
    if (n == "sbx_slice_stats") return sizeof(sbx_slice_stats);
    if (n == "sbx_import_stats") return sizeof(sbx_import_stats);
    if (n == "sbx_fixbins_stats") return sizeof(sbx_fixbins_stats);
    if (n == "sbx_fasta_stats") return sizeof(sbx_fasta_stats);
    if (n == "sbx_view_request") return sizeof(sbx_view_request);
    if (n == "sbx_validate_report") return sizeof(sbx_validate_report);
    if (n == "sbx_validate_stats") return sizeof(sbx_validate_stats);
    if (n == "sbx_view_index_stats") return sizeof(sbx_view_index_stats);
    if (n == "sbx_stream_stats") return sizeof(sbx_stream_stats);
    if (n == "sbx_subsample_stats") return sizeof(sbx_subsample_stats);
    return 0;
}

int sbx_inflate_blocks(const uint8_t* comp, const uint64_t* comp_off, const uint32_t* comp_len, const uint32_t* isize,
                       uint32_t n_blocks, uint8_t* out, const uint64_t* out_off, char* err, size_t errlen) {
    try {
        require_device(-1);
        if (n_blocks == 0) return SBX_OK;
        uint64_t in_end = 0, out_end = 0;
        for (uint32_t i = 0; i < n_blocks; ++i) {
            in_end = std::max(in_end, comp_off[i] + comp_len[i]);
            out_end = std::max(out_end, out_off[i] + isize[i]);
        }
        DevBuf<uint8_t> d_in(in_end + kCompPad), d_out(out_end + 64), d_scr(inflate_scratch_bytes(n_blocks));
        DevBuf<uint8_t> d_lit(inflate_lit_bytes(out_end, n_blocks));
        DevBuf<uint32_t> d_ent(inflate_ent_words(out_end, n_blocks)), d_nent(n_blocks);
        DevBuf<uint64_t> d_coff(n_blocks), d_ooff(n_blocks);
        DevBuf<uint32_t> d_clen(n_blocks), d_isz(n_blocks), d_st(n_blocks);
        SBX_HIP(hipMemset(d_in.p + in_end, 0, 64));
        SBX_HIP(hipMemcpy(d_in.p, comp, in_end, hipMemcpyHostToDevice));
        // (the caller's bytes between and around the blocks make the round trip through the device buffer: a kernel that wrote outside a
        // block's range would show in them -- tests/test_gpu_inflate_writeout.py)
        SBX_HIP(hipMemcpy(d_out.p, out, out_end, hipMemcpyHostToDevice));
        SBX_HIP(hipMemcpy(d_coff.p, comp_off, n_blocks * 8ull, hipMemcpyHostToDevice));
        SBX_HIP(hipMemcpy(d_ooff.p, out_off, n_blocks * 8ull, hipMemcpyHostToDevice));
        SBX_HIP(hipMemcpy(d_clen.p, comp_len, n_blocks * 4ull, hipMemcpyHostToDevice));
        SBX_HIP(hipMemcpy(d_isz.p, isize, n_blocks * 4ull, hipMemcpyHostToDevice));
        launch_bgzf_inflate(d_in.p, d_coff.p, d_clen.p, d_isz.p, d_ooff.p, d_out.p, n_blocks, 0, d_scr.p, d_lit.p, d_ent.p,
                            d_nent.p, d_st.p, nullptr);
        std::vector<uint32_t> st(n_blocks);
        SBX_HIP(hipMemcpy(st.data(), d_st.p, n_blocks * 4ull, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_blocks; ++i)
            if (st[i]) throw Error(SBX_EFORMAT, "block " + std::to_string(i) + ": " + inflate_status_string(st[i]));
        // (blocks may be sparse in `out`: what lies between them comes back as it went in)
        SBX_HIP(hipMemcpy(out, d_out.p, out_end, hipMemcpyDeviceToHost));
        return SBX_OK;
    } catch (const Error& e) {
        set_err(err, errlen, e.what());
        return e.code;
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        return SBX_EINVAL;
    }
}

int sbx_device_count(void) {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0 ? n : 0;
}

// shares of the concatenated reference (sambamba_amd/shard.py plan_position_shards states the same rule; tests/test_shard_plan_cpu.py
// holds the two against each other)
int sbx_plan_shards(const int64_t* ref_lengths, int32_t n_ref, int32_t n_shards, uint32_t align, sbx_shard* out, size_t cap, size_t* n_out) {
    if (n_out) *n_out = 0;
    if (n_ref < 0 || n_shards < 1 || align == 0 || (n_ref && !ref_lengths)) return SBX_EINVAL;
    std::vector<uint64_t> lens((size_t)n_ref), starts((size_t)n_ref);
    uint64_t total = 0;
    for (int32_t r = 0; r < n_ref; ++r) {
        lens[(size_t)r] = ref_lengths[r] > 0 ? (uint64_t)std::min<int64_t>(ref_lengths[r], 0x7FFFFFFF) : 0;
        starts[(size_t)r] = total;
        total += lens[(size_t)r];
    }
    if (total == 0) return SBX_OK;
    struct Cut { uint32_t ref; uint64_t pos; };
    auto less = [](const Cut& a, const Cut& b) { return a.ref != b.ref ? a.ref < b.ref : a.pos < b.pos; };
    std::vector<Cut> bounds((size_t)n_shards + 1);
    bounds[0] = {0, 0};
    for (int32_t k = 1; k < n_shards; ++k) {
        const uint64_t g = (uint64_t)((unsigned __int128)total * (uint64_t)k / (uint64_t)n_shards);      // 0 <= g < total
        const size_t r = (size_t)(std::upper_bound(starts.begin(), starts.end(), g) - starts.begin()) - 1;
        bounds[(size_t)k] = {(uint32_t)r, (g - starts[r]) / align * align};
        if (less(bounds[(size_t)k], bounds[(size_t)k - 1])) bounds[(size_t)k] = bounds[(size_t)k - 1];   // monotone (tiny contigs, more shards than tiles)
    }
    bounds[(size_t)n_shards] = {(uint32_t)n_ref, 0};
    size_t n = 0;
    for (int32_t k = 0; k < n_shards; ++k) {
        const Cut a = bounds[(size_t)k], b = bounds[(size_t)k + 1];
        for (uint32_t r = a.ref; r <= std::min<uint32_t>(b.ref, (uint32_t)n_ref - 1); ++r) {
            const uint64_t beg = r == a.ref ? a.pos : 0, end = r == b.ref ? b.pos : lens[r];
            if (end > beg) {
                if (out && n < cap) out[n] = {(uint32_t)k, r, (uint32_t)beg, (uint32_t)end};
                ++n;
            }
        }
    }
    if (n_out) *n_out = n;
    return (out && n <= cap) || (!out && cap == 0) ? SBX_OK : SBX_ENOMEM;
}

sbx_ctx* sbx_open(const char* const* bam_paths, int n_bams, int device, char* err, size_t errlen) {
    std::unique_ptr<sbx_ctx> c(new sbx_ctx());
    try {
        if (n_bams < 1 || !bam_paths || !bam_paths[0]) throw Error(SBX_EINVAL, "no input files");
        const bool timing = getenv("SBX_TIMING") != nullptr;
        const double t0 = wall_now();
        // the host side of opening -- mapping the file, the BAI, the scan of the BGZF headers -- runs next to the bring-up of the
        // HIP runtime (80 ms for a process's first HIP call)
        std::exception_ptr host_err;
        bool host_joined = false;
        std::thread host([&] {
            try {
                c->file.open(bam_paths[0]);
                c->has_index = load_bai(c->file.path, &c->bai);
                // every virtual offset of the index names a BGZF block start: the header chain is scanned in pieces
                std::vector<uint64_t> hints;
                for (auto& r : c->bai.refs) {
                    for (uint64_t v : r.ioffsets) hints.push_back(v >> 16);
                    for (auto& b : r.bins) for (auto& ch : b.chunks) hints.push_back(ch.beg >> 16);
                }
                c->blocks = scan_bgzf(c->file.data, c->file.size, hints.empty() ? nullptr : &hints);
            } catch (...) { host_err = std::current_exception(); }
        });
        struct Joiner { std::thread& t; bool& done; ~Joiner() { if (!done && t.joinable()) t.join(); } } joiner{host, host_joined};
        require_device(device);
        SBX_HIP(hipGetDevice(&c->device));
        c->stream.create();
        c->copy_stream.create();
        c->text_stream.create();
        const double t1 = wall_now();
        host.join();
        host_joined = true;
        if (host_err) std::rethrow_exception(host_err);
        const double t2 = t1;
        default_filter(&c->filter);
        const double t3 = wall_now();
        parse_header_on_device(c.get());
        if (timing)
            fprintf(stderr, "[sbx] open %s: device (with the BAI and the BGZF scan of %zu blocks next to it) %.3f s, wait for the scan %.3f s, header %.3f s\n",
                    bam_paths[0], c->blocks.size(), t1 - t0, t3 - t2, wall_now() - t3);
        // further files: MultiBamReader semantics that matter for depth -- identical reference dictionaries
        // (the reference merges compatible ones, multireader.d:174-215; anything else is rejected here), samples =
        // union of the @RG SM values in order of first appearance (depth.d:1170-1181 over the merged header), every
        // file keeps its own RG-id -> sample table (so colliding RG ids need no renaming)
        for (int i = 1; i < n_bams; ++i) {
            if (!bam_paths[i]) throw Error(SBX_EINVAL, "null path");
            const char* one[1] = {bam_paths[i]};
            char e2[512] = {0};
            sbx_ctx* m = sbx_open(one, 1, c->device, e2, sizeof e2);
            if (!m) throw Error(SBX_EIO, e2);
            c->members.push_back(m);
            m->in_group = true;
            c->in_group = true;
            if (m->hdr.sorting_order != "coordinate") c->hdr.sorting_order = m->hdr.sorting_order;
            if (!m->has_index) c->has_index = false;
        }
        if (!c->members.empty()) {
            // the reference dictionary of the merged header (SamHeaderMerger); files whose own dictionary differs from it translate
            // the reference ids of their records on the device (RefTable::own_to_merged) and the ids of BAI queries on the host
            {
                const auto files = files_of(c.get());
                std::vector<const std::vector<RefSeq>*> dicts;
                for (sbx_ctx* f : files) dicts.push_back(&f->hdr.refs);
                std::vector<RefSeq> merged;
                std::vector<std::vector<int32_t>> maps;
                merge_dictionaries(dicts, &merged, &maps);
                for (size_t k = 0; k < files.size(); ++k) {
                    sbx_ctx* f = files[k];
                    bool same = f->hdr.refs.size() == merged.size();
                    for (size_t r = 0; same && r < merged.size(); ++r) same = maps[k][r] == (int32_t)r;
                    if (same) continue;
                    f->own_to_merged = maps[k];
                    f->merged_to_own.assign(merged.size(), -1);
                    for (size_t r = 0; r < maps[k].size(); ++r) f->merged_to_own[(size_t)maps[k][r]] = (int32_t)r;
                    f->hdr.refs = merged;
                }
            }
            std::vector<std::string> names;
            auto id_of = [&](const std::string& sm) -> uint16_t {
                for (size_t k = 0; k < names.size(); ++k) if (names[k] == sm) return (uint16_t)k;
                names.push_back(sm);
                return (uint16_t)(names.size() - 1);
            };
            for (sbx_ctx* f : files_of(c.get())) {
                f->hdr.rg_sample.clear();
                for (auto& g : f->hdr.read_groups) f->hdr.rg_sample.push_back(id_of(g.sample));
            }
            if (names.empty()) names.push_back("*");
            for (sbx_ctx* f : files_of(c.get())) f->hdr.sample_names = names;
        }
        return c.release();
    } catch (const std::exception& e) {
        set_err(err, errlen, e.what());
        const Error* x = dynamic_cast<const Error*>(&e);
        t_open_code = x ? x->code : SBX_EINVAL;
        if (c) for (sbx_ctx* m : c->members) sbx_close(m);
        return nullptr;
    }
}

void sbx_close(sbx_ctx* c) {
    if (!c) return;
    for (sbx_ctx* m : c->members) sbx_close(m);
    delete c;       // (the streams wait for their work and go first: engine_ctx.hpp)
}

const char* sbx_last_error(sbx_ctx* c) {
    if (!c) return "null context";
    // (a prefetch on a second thread may set the message while this one reads it: the caller gets its own copy)
    static thread_local std::string copy;
    std::lock_guard<std::mutex> g(c->err_mu);
    copy = c->last_error;
    return copy.c_str();
}

int sbx_header(sbx_ctx* c, sbx_header_info* out) {
    if (!c || !out) return SBX_EINVAL;
    out->n_ref = (int32_t)c->hdr.refs.size();
    out->n_samples = (int32_t)c->hdr.sample_names.size();
    out->n_read_groups = (int32_t)c->hdr.read_groups.size();
    out->sorted_by_coordinate = c->hdr.sorting_order == "coordinate";
    out->has_index = c->has_index ? 1 : 0;
    out->reserved = 0;
    out->n_bgzf_blocks = c->blocks.size();
    out->compressed_bytes = c->file.size;
    out->uncompressed_bytes = c->blocks.out_off.back();
    return SBX_OK;
}
const char* sbx_ref_name(sbx_ctx* c, int r) { return (c && r >= 0 && (size_t)r < c->hdr.refs.size()) ? c->hdr.refs[(size_t)r].name.c_str() : nullptr; }
int64_t sbx_ref_length(sbx_ctx* c, int r) { return (c && r >= 0 && (size_t)r < c->hdr.refs.size()) ? c->hdr.refs[(size_t)r].length : -1; }
int sbx_ref_id(sbx_ctx* c, const char* name) { return (c && name) ? c->hdr.find_ref(name) : -1; }
const char* sbx_sample_name(sbx_ctx* c, int s) { return (c && s >= 0 && (size_t)s < c->hdr.sample_names.size()) ? c->hdr.sample_names[(size_t)s].c_str() : nullptr; }
const char* sbx_header_text(sbx_ctx* c, size_t* len) {
    if (!c) return nullptr;
    if (len) *len = c->hdr.text.size();
    return c->hdr.text.c_str();
}

int sbx_compile_filter(const char* query, sbx_filter* out, char* err, size_t errlen) {
    if (!out) return SBX_EINVAL;
    try {
        memset(out, 0, sizeof *out);
        if (!query) default_filter(out);
        else { FilterCompiler fc(query, out); fc.compile(); }
        return SBX_OK;
    } catch (const Error& e) {
        set_err(err, errlen, e.what());
        return e.code;
    }
}

int sbx_regex_search(const char* pattern, const char* options, const char* text, size_t n, char* err, size_t errlen) {
    if (!pattern || (!text && n)) return SBX_EINVAL;
    try {
        bool icase = false;
        for (const char* o = options; o && *o; ++o) {
            if (*o == 'i') icase = true;
            else throw Error(SBX_EUNSUPPORTED, std::string("filter: regular expression option '") + *o + "' is not supported on the device path");
        }
        sbx_regex re;
        RegexCompiler rc(pattern, icase, &re);
        rc.compile();
        return re_search(re, (uint32_t)n, [&](uint32_t k) { return (uint8_t)text[k]; }) ? 1 : 0;
    } catch (const Error& e) {
        set_err(err, errlen, e.what());
        return e.code;
    }
}

int sbx_set_filter(sbx_ctx* c, const sbx_filter* f) {
    if (!c || !f || f->n_ops < 0 || f->n_ops > SBX_FILTER_MAX_OPS) return SBX_EINVAL;
    for (sbx_ctx* m : files_of(c)) { m->filter = *f; m->have_run = false; }
    return SBX_OK;
}

int sbx_set_params(sbx_ctx* c, int mode, uint8_t min_bq, int fix_mate, int combined, uint32_t window, uint32_t overlap,
                   const uint32_t* thr, int n_thr) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        if (mode < 0 || mode > 2) throw Error(SBX_EINVAL, "unknown mode");
        if (mode == SBX_MODE_WINDOW) {
            if (window == 0) throw Error(SBX_EINVAL, "positive window size must be specified");        // depth.d:1020-1021
            if (overlap >= window) throw Error(SBX_EINVAL, "specified overlap is larger than window size");  // depth.d:1023-1024
        }
        for (sbx_ctx* m : files_of(c)) {
            m->mode = mode;
            m->min_bq = min_bq;
            m->fix_mate = fix_mate != 0;
            m->combined = combined != 0;
            m->window = window;
            m->overlap = overlap;
            m->thresholds.assign(thr, thr + (n_thr > 0 ? n_thr : 0));
            m->have_run = false;
        }
    });
}

int sbx_set_regions(sbx_ctx* c, const sbx_region* r, size_t n) {
    return guarded(c, [&] {
        if (!c) throw Error(SBX_EINVAL, "null context");
        for (size_t i = 0; i < n; ++i) {
            if (r[i].ref_id >= c->hdr.refs.size()) throw Error(SBX_EINVAL, "Invalid reference sequence index");
            if (!(r[i].start < r[i].end)) throw Error(SBX_EINVAL, "Enforcement failed");   // randomaccessmanager.d:256
        }
        for (sbx_ctx* m : files_of(c)) { m->regions.assign(r, r + n); m->have_run = false; }
    });
}

// -L argument -> regions, exactly as depth_main does it (depth.d:1184-1208): a BED file (bed.d:59-152), or, when it
// cannot be read as one, a region string (BioD/bio/core/region.d:97-246).
int sbx_parse_regions(sbx_ctx* c, const char* arg, size_t* n_merged, size_t* n_raw) {
    return guarded(c, [&] {
        if (!c || !arg) throw Error(SBX_EINVAL, "null argument");
        c->parsed_merged.clear(); c->parsed_raw.clear(); c->parsed_lines.clear();
        std::vector<BedInterval> ivs;
        std::vector<std::string> lines;
        std::vector<size_t> line_of;
        if (read_bed_file(arg, &ivs, &lines, &line_of)) {
            c->parsed_merged = bed_merged(ivs, c->hdr);
            // every kept region keeps its own input line (the reference pairs them by index, which misaligns when a
            // line names a contig the BAM does not have -- SURVEY App. B-6)
            for (size_t i = 0; i < ivs.size(); ++i) {
                const int id = c->hdr.find_ref(ivs[i].chr);
                if (id < 0) continue;
                c->parsed_raw.push_back({(uint32_t)id, (uint32_t)ivs[i].beg, (uint32_t)ivs[i].end});
                c->parsed_lines.push_back(lines[line_of[i]]);
            }
        } else {
            const RegionString rs = parse_region_string(arg);
            const int id = c->hdr.find_ref(rs.reference);
            if (id < 0) throw Error(SBX_EINVAL, std::string("couldn't open file ") + arg + " or find reference " + rs.reference);
            sbx_region g{(uint32_t)id, rs.beg, rs.end};
            if (g.end == 0xFFFFFFFFu) g.end = (uint32_t)c->hdr.refs[(size_t)id].length;
            c->parsed_merged.push_back(g);
            c->parsed_raw.push_back(g);
            c->parsed_lines.push_back(rs.reference + "\t" + std::to_string(g.start) + "\t" + std::to_string(g.end));
        }
        if (n_merged) *n_merged = c->parsed_merged.size();
        if (n_raw) *n_raw = c->parsed_raw.size();
    });
}
int sbx_parsed_regions(sbx_ctx* c, int merged, sbx_region* out, size_t cap) {
    if (!c || (!out && cap)) return SBX_EINVAL;
    const auto& v = merged ? c->parsed_merged : c->parsed_raw;
    if (cap < v.size()) return SBX_ENOMEM;
    for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    return SBX_OK;
}
const char* sbx_parsed_region_line(sbx_ctx* c, size_t raw_index) {
    return (c && raw_index < c->parsed_lines.size()) ? c->parsed_lines[raw_index].c_str() : nullptr;
}

int sbx_last_run_stats(sbx_ctx* c, sbx_run_stats* out) {
    if (!c || !out) return SBX_EINVAL;
    *out = c->stats;
    return SBX_OK;
}

// extent of the tile grid of a contig (positions) and activity of a tile -- used by the CLI to skip
// empty stretches without copying zeros.
int sbx_tile_info(sbx_ctx* c, uint32_t* tile_pos, uint32_t* n_samples) {
    if (!c || !c->have_run) return SBX_EINVAL;
    if (tile_pos) *tile_pos = c->tile_pos;
    if (n_samples) *n_samples = c->n_samples_eff;
    return SBX_OK;
}
// next active tile of ref_id at or after position `from`; returns its [beg,end) or beg==end==UINT32_MAX
int sbx_next_active_range(sbx_ctx* c, uint32_t ref_id, uint64_t from, uint64_t* beg, uint64_t* end) {
    if (!c || !c->have_run || ref_id >= c->hdr.refs.size() || !beg || !end) return SBX_EINVAL;
    const uint32_t T = c->tile_pos;
    const uint32_t t_first = c->h_tile_base[ref_id], t_end = c->h_tile_base[ref_id + 1];
    uint64_t t = t_first + from / T;
    while (t < t_end && c->h_slot_of[(size_t)t] == 0xFFFFFFFFu) ++t;
    if (t >= t_end) { *beg = *end = ~0ULL; return SBX_OK; }
    uint64_t t2 = t;
    while (t2 < t_end && c->h_slot_of[(size_t)t2] != 0xFFFFFFFFu) ++t2;
    *beg = std::max<uint64_t>(from, (t - t_first) * (uint64_t)T);
    *end = (t2 - t_first) * (uint64_t)T;
    return SBX_OK;
}

}  // extern "C"
