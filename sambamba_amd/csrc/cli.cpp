// cli.cpp -- `sbx-depth`: the host side of `sambamba depth base|region|window` on top of the
// C ABI of libsbx_depth.so.  It mirrors depth_main (sambamba/depth.d:1079-1245): same
// sub-commands, same options (depth.d:59-98), same text output byte for byte, same error
// line ("sambamba-depth: <msg>", exit code 1).  All counting happens on the MI355X through
// sbx_run(); this file only parses arguments and prints.
//
//   sbx-depth base   [-F filter] [-o out] [-c min] [-C max] [-q bq] [-a] [--combined] [-L regions] [-z] in.bam
//   sbx-depth region -L regions [-T thr]... [common options] in.bam
//   sbx-depth window -w size [--overlap n] [-T thr]... [common options] in.bam
//
// This file: usage, the option policy (the scanner is cli_opts.hpp), depth_main -- parse, validate, header line, devices, open, regions,
// choose the path, ONE way out -- and the process model (main).  The printers and the paths are cli_base / _stats / _pipeline / _sharded.hpp.
#include <cerrno>
#include <csignal>
#include <fcntl.h>
#include <sys/prctl.h>
#include <sys/wait.h>
#include <unistd.h>

#include "host_io.hpp"
#include "cli_opts.hpp"
#include "cli_pipeline.hpp"
#include "cli_sharded.hpp"

using namespace sbx;

namespace {

void usage() {  // depth.d:50-99
    fputs("Usage: sambamba-depth region|window|base [options] input.bam  [input2.bam [...]]\n\n"
          "          All BAM files must be coordinate-sorted and indexed.\n\n"
          "          The tool has three modes: base, region, and window,\n"
          "          each name means per which unit to print the statistics.\n\n"
          "Common options:\n"
          "         -F, --filter=FILTER\n"
          "                    set custom filter for alignments; the default value is\n"
          "                    'mapping_quality > 0 and not duplicate and not failed_quality_control'\n"
          "         -o, --output-file=FILENAME\n"
          "                    output filename (by default /dev/stdout)\n"
          "         -t, --nthreads=NTHREADS\n"
          "                    maximum number of threads to use\n"
          "         -c, --min-coverage=MINCOVERAGE\n"
          "                    minimum mean coverage for output (default: 0 for region/window, 1 for base)\n"
          "         -C, --max-coverage=MAXCOVERAGE\n"
          "                    maximum mean coverage for output\n"
          "         -q, --min-base-quality=QUAL\n"
          "                    don't count bases with lower base quality\n"
          "         --combined\n"
          "                    output combined statistics for all samples\n"
          "         -a, --annotate\n"
          "                    add additional column of y/n instead of\n"
          "                    skipping records not satisfying the criteria\n"
          "         -m, --fix-mate-overlaps\n"
          "                    detect overlaps of mate reads and handle them on per-base basis\n"
          "base subcommand options:\n"
          "         -L, --regions=FILENAME|REGION\n"
          "                    list or regions of interest or a single region in form chr:beg-end (optional)\n"
          "         -z, --report-zero-coverage (DEPRECATED, use --min-coverage=0 instead)\n"
          "                    don't skip zero coverage bases\n"
          "region subcommand options:\n"
          "         -L, --regions=FILENAME|REGION\n"
          "                    list or regions of interest or a single region in form chr:beg-end (required)\n"
          "         -T, --cov-threshold=COVTHRESHOLD\n"
          "                    multiple thresholds can be provided,\n"
          "                    for each one an extra column will be added,\n"
          "                    the percentage of bases in the region\n"
          "                    where coverage is more than this value\n"
          "window subcommand options:\n"
          "         -w, --window-size=WINDOWSIZE\n"
          "                    breadth of the window, in bp (required)\n"
          "         --overlap=OVERLAP\n"
          "                    overlap of successive windows, in bp (default is 0)\n"
          "         -T, --cov-threshold=COVTHRESHOLD\n"
          "                    same meaning as in 'region' subcommand\n",
          stderr);
}

// The policy of sbx-depth is D getopt's with passThrough: what the table does not name -- `--xyz`, `-x`, a bare `--` -- is a
// positional (that is how `--no-such-option` becomes a file name), a flag with text attached (`-afoo`, `--annotate=1`) is still
// that flag, and numbers go through atoi / atof / strtoul unvalidated.
enum { kFilter, kOutput, kThreads, kMinCov, kMaxCov, kMinBq, kAnnotate, kCombined, kFixMate, kRegions, kReportZero, kThreshold, kWindow, kOverlap, kGpus };
bool parse_args(int argc, char** argv, Options* o, std::string* err) {
    o->mode = argv[1];
    if (o->mode == "base") o->min_cov = 1;  // depth.d:1113-1114
    static const OptSpec specs[] = {
        {"filter", 'F', true, kFilter}, {"output-filename", 'o', true, kOutput}, {"nthreads", 't', true, kThreads},
        {"min-coverage", 'c', true, kMinCov}, {"max-coverage", 'C', true, kMaxCov}, {"min-base-quality", 'q', true, kMinBq},
        {"annotate", 'a', false, kAnnotate}, {"combined", 0, false, kCombined}, {"fix-mate-overlaps", 'm', false, kFixMate},
        {"regions", 'L', true, kRegions}, {"report-zero-coverage", 'z', false, kReportZero}, {"cov-threshold", 'T', true, kThreshold},
        {"window-size", 'w', true, kWindow}, {"overlap", 0, true, kOverlap}, {"gpus", 0, true, kGpus}};
    for (int i = 2; i < argc; ++i) {
        const OptToken t = next_opt(argc, argv, &i, specs);
        if (t.kind != OptToken::Option) { o->bams.push_back(t.arg); continue; }
        if (t.missing) { *err = "Missing value for argument " + t.arg + "."; return false; }
        const char* val = t.value.c_str();
        switch (t.spec->id) {
        case kFilter: o->filter = t.value; o->has_filter = true; break;
        case kOutput: o->output_fn = t.value; break;
        case kThreads: o->n_threads = atoi(val); break;
        case kMinCov: o->min_cov = atof(val); break;
        case kMaxCov: o->max_cov = atof(val); break;
        case kMinBq: o->min_bq = atoi(val); break;
        case kAnnotate: o->annotate = true; break;
        case kCombined: o->combined = true; break;
        case kFixMate: o->fix_mate = true; break;
        case kRegions: o->regions = t.value; o->has_regions = true; break;
        case kReportZero: o->report_zero = true; break;
        case kThreshold: o->thresholds.push_back((uint32_t)strtoul(val, nullptr, 10)); break;
        case kWindow: o->window = strtoull(val, nullptr, 10); break;
        case kOverlap: o->overlap = strtoull(val, nullptr, 10); break;
        case kGpus: o->gpus = atoi(val); break;
        }
    }
    if (o->mode == "window") o->has_regions = false;  // -L is not parsed in window mode (depth.d:1139)
    return true;
}

// (detached mode, see main) tells the waiting parent that the output is complete: everything buffered is written, the
// standard descriptors are closed -- a consumer on a pipe sees end-of-file now, not after the teardown -- and the status sent
int g_done_fd = -1;
void report_done(int rc) {
    if (g_done_fd < 0) return;
    fflush(nullptr);
    prctl(PR_SET_PDEATHSIG, 0);
    close(0); close(1); close(2);
    const unsigned char st = (unsigned char)rc;
    ssize_t n;
    do n = write(g_done_fd, &st, 1); while (n < 0 && errno == EINTR);
    close(g_done_fd);
    g_done_fd = -1;
}

struct Job {      // what depth_main has set up by the time it chooses how to run
    Options o;
    Out out;
    sbx_ctx* ctx = nullptr;
    sbx_header_info hi;
    sbx_filter filt;
    int mode_id = SBX_MODE_BASE;
    std::vector<const char*> paths;
    std::vector<std::string> samples, raw_lines;
    std::vector<sbx_region> merged, raw;      // -L: merged for the device, raw (file order) with the input line of each (raw_lines)
    std::vector<sbx_batch> plan;
    bool timing = false;                      // SBX_TIMING: phase wall clock on stderr (profiles/, tools/cli_e2e.sh)
    double t_start = 0, t_open = 0;
};

// The one way out of a run that succeeded: the output is flushed and closed, then the process ends -- device memory, mappings and
// streams go with it (an orderly sbx_close frees tens of gigabytes buffer by buffer and costs 0.1 s that no caller is waiting
// for) -- or, with SBX_ORDERLY_EXIT, the contexts are closed and depth_main returns.  `line(when, t_out)` prints the SBX_TIMING
// line of the path at the moment(s) it wants to.
enum class Exit { WithoutFreeing, BeforeClose, AfterClose };
template <class F> int finish_run(Job& j, const std::vector<sbx_ctx*>& others, F&& line) {
    j.out.flush();
    if (j.out.fp != stdout) fclose(j.out.fp);
    const double t_out = now();
    const bool orderly = getenv("SBX_ORDERLY_EXIT") != nullptr;
    if (j.timing) line(orderly ? Exit::BeforeClose : Exit::WithoutFreeing, t_out);
    if (!orderly) { fflush(nullptr); report_done(0); _exit(0); }
    for (sbx_ctx* c : others) if (c) sbx_close(c);
    sbx_close(j.ctx);
    if (j.timing) line(Exit::AfterClose, t_out);
    return 0;
}

// --gpus N / SBX_DEVICES=a,b,...: the devices of a sharded job (an ordinal may repeat: several contexts on one device -- how the
// sharded path is tested on a one-GPU box)
std::vector<int> job_devices(const Options& o) {
    std::vector<int> devices;
    if (const char* e = getenv("SBX_DEVICES")) {
        for (const char* q = e; *q;) {
            char* end = nullptr;
            const long v = strtol(q, &end, 10);
            if (end == q || v < 0) throw Fail{std::string("SBX_DEVICES: a comma-separated list of device ordinals is expected, got '") + e + "'"};
            devices.push_back((int)v);
            q = *end == ',' ? end + 1 : end;
            if (*end && *end != ',') throw Fail{std::string("SBX_DEVICES: a comma-separated list of device ordinals is expected, got '") + e + "'"};
        }
        if (o.gpus > 0 && (size_t)o.gpus < devices.size()) devices.resize((size_t)o.gpus);
    } else if (o.gpus > 1) {
        const int have = sbx_device_count();
        if (o.gpus > have) throw Fail{"--gpus " + std::to_string(o.gpus) + ": " + std::to_string(have) + " HIP device(s) visible"};
        for (int k = 0; k < o.gpus; ++k) devices.push_back(k);
    }
    return devices;
}

// -L (depth.d:1184-1212)
void read_regions(Job& j) {
    const Options& o = j.o;
    sbx_ctx* ctx = j.ctx;
    // host-side header view for BED contig lookups
    BamHeaderInfo hv;
    for (int r = 0; r < j.hi.n_ref; ++r) hv.refs.push_back({sbx_ref_name(ctx, r), (int32_t)sbx_ref_length(ctx, r)});
    std::vector<BedInterval> ivs;
    std::vector<std::string> lines;
    std::vector<size_t> line_of;
    if (read_bed_file(o.regions, &ivs, &lines, &line_of)) {
        j.merged = bed_merged(ivs, hv);
        // raw list in file order; every kept region keeps its own input line (the reference
        // pairs them by index, which misaligns when a line is dropped -- SURVEY App. B-6)
        for (size_t i = 0; i < ivs.size(); ++i) {
            int id = hv.find_ref(ivs[i].chr);
            if (id < 0) continue;
            j.raw.push_back({(uint32_t)id, (uint32_t)ivs[i].beg, (uint32_t)ivs[i].end});
            j.raw_lines.push_back(lines[line_of[i]]);
        }
        if (o.mode == "region" && lines.empty()) throw Fail{"Attempting to fetch the front of an empty array of string"};
    } else {
        RegionString rs = parse_region_string(o.regions);
        int id = sbx_ref_id(ctx, rs.reference.c_str());
        if (id < 0) throw Fail{"couldn't open file " + o.regions + " or find reference " + rs.reference};
        sbx_region g{(uint32_t)id, rs.beg, rs.end};
        if (g.end == 0xFFFFFFFFu) g.end = (uint32_t)sbx_ref_length(ctx, id);
        j.merged.push_back(g);
        j.raw.push_back(g);
        j.raw_lines = {rs.reference + "\t" + std::to_string(g.start) + "\t" + std::to_string(g.end)};
    }
    if (j.merged.empty()) throw Fail{"Enforcement failed"};
    check(ctx, sbx_set_regions(ctx, j.merged.data(), j.merged.size()));
}

// Can this option set run sharded by position?  Not when the output depends on the order of the whole stream.
bool can_shard(const Job& j, const BasePrinter& bp) {
    const Options& o = j.o;
    if (o.mode == "base") return !o.has_regions && o.min_cov > 0 && bp.device_format_applies();
    if (o.mode == "region") return true;
    const uint32_t S_eff = o.combined ? 1u : (uint32_t)j.samples.size();
    uint64_t total_win = 0;
    for (int r = 0; r < j.hi.n_ref; ++r) total_win += ref_len(j.ctx, r) / o.window;
    return o.overlap == 0 && total_win * S_eff * (2 + std::max<size_t>(1, o.thresholds.size())) <= (1ull << 28);
}

// several devices: the job sharded by position, one context per device (cli_sharded.hpp)
int run_sharded(Job& j, const std::vector<int>& devices) {
    const Options& o = j.o;
    Sharded sh{o, j.out, j.paths, j.filt, j.mode_id, devices, j.ctx, j.samples, o.mode == "region" ? j.merged : std::vector<sbx_region>{}};
    if (o.mode == "base") sh.base();
    else if (o.mode == "region") {
        RegionPrinter rp{j.ctx, o, j.out, j.samples, j.raw, j.raw_lines};
        sh.region(rp);
        rp.finish();
    } else {
        WindowData wd;
        WindowPrinter wp{j.ctx, o, j.out, j.samples};
        sh.window(wp, wd);
        wp.data = &wd;
        wp.run_refs(0, j.hi.n_ref);
        wp.finish();
    }
    return finish_run(j, std::vector<sbx_ctx*>(sh.cx.begin() + 1, sh.cx.end()), [&](Exit when, double) { if (when != Exit::AfterClose) sh.report(j.t_start); });
}

// The device processes the file in batches of contigs sized to its free memory (one batch unless the
// BAM is whole-genome sized); the printers are fed batch by batch, in contig order.
int run_one_pass(Job& j, BasePrinter& bp) {
    const Options& o = j.o;
    sbx_ctx* ctx = j.ctx;
    double t_run = 0, t_print = 0;
    WindowPrinter wp{ctx, o, j.out, j.samples};
    RegionPrinter rp{ctx, o, j.out, j.samples, j.raw, j.raw_lines};
    for (auto& b : j.plan) {
        const double t0 = now();
        if (j.plan.size() == 1) check(ctx, sbx_run(ctx));
        else check(ctx, sbx_run_batch(ctx, b.first_ref, b.n_refs));
        const double t1 = now();
        const int r0 = (int)b.first_ref, r1 = (int)(b.first_ref + b.n_refs);
        // "Processing reference #N (name)" lines go to stderr in the reference (depth.d:1225-1229)
        if (o.mode == "region") rp.run_refs(r0, r1);
        else if (o.mode == "window") wp.run_refs(r0, r1);
        else bp.run_refs(r0, r1);
        t_run += t1 - t0;
        t_print += now() - t1;
        if (j.timing) {
            sbx_run_stats st;
            if (sbx_last_run_stats(ctx, &st) == SBX_OK)
                fprintf(stderr, "[sbx-depth] batch refs [%d,%d): run %.3f s (h2d %.1f ms, device %.1f ms: inflate %.1f index %.1f accumulate %.1f), %llu records\n",
                        r0, r1, t1 - t0, st.ms_h2d, st.ms_total, st.ms_inflate, st.ms_index, st.ms_accumulate, (unsigned long long)st.n_records);
        }
    }
    if (o.mode == "region") rp.finish();
    else if (o.mode == "window") wp.finish();
    else if (o.mode == "base") bp.finish();
    return finish_run(j, {}, [&](Exit when, double t_out) {
        if (when == Exit::WithoutFreeing)
            fprintf(stderr, "[sbx-depth] open %.3f s, run %.3f s, print %.3f s, finish %.3f s, total %.3f s since main (exit without freeing)\n",
                    j.t_open - j.t_start, t_run, t_print, t_out - j.t_open - t_run - t_print, now() - j.t_start);
        else if (when == Exit::AfterClose)
            fprintf(stderr, "[sbx-depth] open %.3f s, run %.3f s, print %.3f s, finish %.3f s, close %.3f s, total %.3f s since main\n",
                    j.t_open - j.t_start, t_run, t_print, t_out - j.t_open - t_run - t_print, now() - t_out, now() - j.t_start);
    });
}

int die(Job& j, const char* msg) {
    j.out.flush();
    fprintf(stderr, "sambamba-depth: %s\n", msg);
    if (j.ctx) sbx_close(j.ctx);
    return 1;
}

int depth_main(int argc, char** argv) {
    if (argc < 3) { usage(); return 0; }
    std::string mode = argv[1];
    if (mode != "base" && mode != "region" && mode != "window") { usage(); return 0; }
    Job j;
    Options& o = j.o;
    Out& out = j.out;
    sbx_ctx*& ctx = j.ctx;
    std::string perr;
    if (!parse_args(argc, argv, &o, &perr)) { fprintf(stderr, "sambamba-depth: %s\n", perr.c_str()); return 1; }
    if (o.mode == "region" && !o.has_regions) {
        fputs("BED file or a region must be provided in region mode\n", stderr);
        return 1;
    }
    try {
        if (!o.output_fn.empty()) {
            out.fp = fopen(o.output_fn.c_str(), "w+");
            if (!out.fp) throw Fail{"Cannot open file `" + o.output_fn + "' in mode `w+' (No such file or directory)"};
        }
        if (o.mode == "base" && o.report_zero) o.min_cov = 0;  // PerBasePrinter.init (depth.d:412-427)
        if (o.mode == "window") {
            if (!(o.window > 0)) throw Fail{"positive window size must be specified"};
            if (!(o.overlap < o.window)) throw Fail{"specified overlap is larger than window size"};
        }
        char ebuf[512] = {0};
        if (sbx_compile_filter(o.has_filter ? o.filter.c_str() : nullptr, &j.filt, ebuf, sizeof ebuf) != SBX_OK) throw Fail{ebuf};
        if (o.bams.empty()) throw Fail{"no input files"};
        for (auto& b : o.bams) j.paths.push_back(b.c_str());
        // The header line is printed by printer.init() before the BAM is opened (depth.d:1152),
        // except in region mode where it needs the first BED line (setBed, depth.d:912-923).
        if (o.mode == "base") print_base_header(out, o);
        else if (o.mode == "window") print_bed_header(out, o, 3);   // PerWindowPrinter.init (depth.d:1036)
        j.timing = getenv("SBX_TIMING") != nullptr;
        j.t_start = now();
        const std::vector<int> devices = job_devices(o);
        ctx = sbx_open(j.paths.data(), (int)j.paths.size(), devices.empty() ? -1 : devices[0], ebuf, sizeof ebuf);
        if (!ctx) throw Fail{ebuf};
        j.t_open = now();
        check(ctx, sbx_header(ctx, &j.hi));
        if (!j.hi.sorted_by_coordinate) throw Fail{"All files must be coordinate-sorted"};
        if (!j.hi.has_index) throw Fail{"All files must be indexed"};
        for (int s = 0; s < j.hi.n_samples; ++s) j.samples.push_back(sbx_sample_name(ctx, s));
        j.mode_id = o.mode == "base" ? SBX_MODE_BASE : o.mode == "region" ? SBX_MODE_REGION : SBX_MODE_WINDOW;
        configure_context(ctx, j.filt, j.mode_id, o, nullptr);
        if (o.has_regions) read_regions(j);
        if (o.mode == "region") print_bed_header(out, o, split_ws(j.raw_lines.empty() ? std::string("a b c") : j.raw_lines[0]).size());
        const uint64_t budget = getenv("SBX_BATCH_BYTES") ? strtoull(getenv("SBX_BATCH_BYTES"), nullptr, 10) : 0;
        size_t n_batches = 0;
        check(ctx, sbx_plan_batches(ctx, budget, nullptr, 0, &n_batches));
        j.plan.resize(n_batches);
        if (n_batches) check(ctx, sbx_plan_batches(ctx, budget, j.plan.data(), j.plan.size(), &n_batches));
        BasePrinter bp(ctx, o, out, j.samples);
        if (o.mode == "base" && o.has_regions) bp.set_bed(j.merged);
        if (devices.size() > 1) {
            if (can_shard(j, bp)) return run_sharded(j, devices);
            fprintf(stderr, "[sbx-depth] --gpus: the output of this option set depends on the order of the whole stream (base -L, base -c 0, "
                            "window --overlap) or would not fit the host: running on one device\n");
        }
        // `depth base` whose text is a pure function of the position, on a file worth it: slices through cli_pipeline.hpp
        if (o.mode == "base" && !o.has_regions && o.min_cov > 0 && bp.device_format_applies() && j.paths.size() == 1 &&
            !getenv("SBX_NO_PIPELINE") && (j.hi.compressed_bytes >= (256u << 20) || getenv("SBX_FORCE_PIPELINE"))) {
            BasePipeline pl{ctx, bp, j.paths, j.filt, j.mode_id, o, g_done_fd >= 0 ? 2u : 1u};
            const BasePipeline::Outcome res = pl.run(j.hi.n_ref);
            if (res == BasePipeline::Failed) throw Fail{pl.sync.failure};
            if (res == BasePipeline::Done)
                return finish_run(j, {pl.cx[1]}, [&](Exit when, double) { if (when != Exit::AfterClose) pl.report(j.t_start, j.t_open); });
            if (j.timing) fprintf(stderr, "[sbx-depth] a slice of the pipeline does not fit the device next to the other context (%s): one pass instead\n", pl.sync.failure.c_str());
        }
        return run_one_pass(j, bp);
    } catch (const Fail& f) { return die(j, f.msg.c_str());
    } catch (const std::exception& e) { return die(j, e.what()); }
}

}  // namespace

// One process by default.  SBX_DETACH=1: the work runs in a child process and this one returns as soon as the child reports that the
// output is complete and its descriptors are closed.  What is left for the child then is the teardown of a HIP process with tens
// of gigabytes mapped -- ~0.3 s inside the driver (measured: the same for an orderly close and for _exit, profiles/round3) -- which
// nothing downstream depends on; but the orphan still holds the device while it goes, and the next command of a shell loop or a
// scheduler would start against its memory: a caller has to ask for that trade.
int main(int argc, char** argv) {
    int fd[2];
    const char* det = getenv("SBX_DETACH");
    if (!det || !*det || *det == '0' || getenv("SBX_NO_DETACH") || pipe(fd) != 0) return depth_main(argc, argv);
    const pid_t self = getpid();
    const pid_t pid = fork();                  // before anything touches HIP: a device context does not survive a fork
    if (pid < 0) { close(fd[0]); close(fd[1]); return depth_main(argc, argv); }
    if (pid == 0) {
        close(fd[0]);
        fcntl(fd[1], F_SETFD, FD_CLOEXEC);
        prctl(PR_SET_PDEATHSIG, SIGTERM);      // a caller that kills the command kills the work
        if (getppid() != self) _exit(1);       // (it died before the line above took effect)
        g_done_fd = fd[1];
        const int rc = depth_main(argc, argv);
        report_done(rc);
        _exit(rc);
    }
    close(fd[1]);
    unsigned char st = 0;
    ssize_t n;
    do n = read(fd[0], &st, 1); while (n < 0 && errno == EINTR);
    if (n == 1) _exit(st);
    int ws = 0;                                // the child ended without a report: its fate is the command's
    while (waitpid(pid, &ws, 0) < 0 && errno == EINTR) {}
    if (WIFSIGNALED(ws)) {                     // killed by a signal (SIGPIPE from a consumer that left, SIGKILL ...): die by the same one
        signal(WTERMSIG(ws), SIG_DFL);
        raise(WTERMSIG(ws));
        return 128 + WTERMSIG(ws);             // (a signal that cannot kill this process)
    }
    return WIFEXITED(ws) ? WEXITSTATUS(ws) : 1;
}
