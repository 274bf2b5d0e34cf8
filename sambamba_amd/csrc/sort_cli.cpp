// sort_cli.cpp -- `sbx-sort`: the command line of `sambamba-sort` (sort_main, sambamba/sort.d:495-576) on top of the C ABI of
// libsbx_depth.so.  Reading, sorting and compressing happen on the device (sbx_sort_bam); this file parses the options.
//
//   sbx-sort [-o OUT|--out=OUT] [-l N|--compression-level=N] [-F FILTER|--filter=FILTER] in.bam
//
// Coordinate order only: -n / --sort-by-name, -N / --natural-sort, --sort-picard and -M / --match-mates are refused.  -m, --tmpdir,
// -u, -t and -p are accepted and ignored: the file is sorted in device memory, there are no chunks on disk and no thread pool.  As with
// D's getopt, options may follow the file name (cli_opts.hpp scans them); `--` ends the options, an option that is not in the table is
// "Unrecognized option X", and so is a short flag with text attached (`-ux`).  Without -o the output is the input with its extension replaced by "sorted.bam"
// (setExtension, sort.d:535); an output that is the input is refused (protectFromOverwrite); like the reference's BamWriter, an
// output whose name ends in ".bam" gets a "<out>.bai" next to it.  Errors: "sbx-sort: <message>" on stderr and exit status 1.
//
// Built once more with -DSBX_SORT_BY_NAME=1 this file is `sbx-nsort`: everything above, and -n / --sort-by-name, -N /
// --natural-sort and -M / --match-mates are taken (sbx_sort_bam_by_name; no .bai for a name order).  -n with -N is the reference's
// "only one of -n and -N and -s parameters can be provided", -M alone its "-M option only works in combination with either -n or
// -N" (sort.d:524-532); --sort-picard stays refused.  Without -n and -N it is sbx-sort.  Errors: "sbx-nsort: <message>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

#ifndef SBX_SORT_BY_NAME
#define SBX_SORT_BY_NAME 0
#endif
#if SBX_SORT_BY_NAME
#define SBX_SORT_PROG "sbx-nsort"
#else
#define SBX_SORT_PROG "sbx-sort"
#endif

namespace {

void usage() {
    fputs("Usage: " SBX_SORT_PROG " [options] <input.bam>\n"
          "\n"
#if SBX_SORT_BY_NAME
          "Sorts a BAM file by coordinate or by read name, as `sambamba sort` does, on the GPU.\n"
#else
          "Sorts a BAM file by coordinate, as `sambamba sort` does, on the GPU.\n"
#endif
          "\n"
          "Options: -o, --out=OUTPUTFILE\n"
          "               output file name; if not provided, the result is written to a file with .sorted.bam extension\n"
          "         -l, --compression-level=COMPRESSION_LEVEL\n"
          "               level of compression for sorted BAM, from 0 to 9\n"
          "         -F, --filter=FILTER\n"
          "               keep only reads that satisfy FILTER\n"
          "         -m, --memory-limit=LIMIT, --tmpdir=TMPDIR, -u, --uncompressed-chunks, -t, --nthreads=NTHREADS, -p, --show-progress\n"
          "               accepted for compatibility; the file is sorted in GPU memory\n"
#if SBX_SORT_BY_NAME
          "         -n, --sort-by-name\n"
          "               sort by read name instead of coordinate (lexicographical order)\n"
          "         -N, --natural-sort\n"
          "               sort by read name instead of coordinate (so-called 'natural' sort as in samtools)\n"
          "         -M, --match-mates\n"
          "               pull mates of the same alignment together when sorting by read name\n"
          "         --sort-picard\n"
          "               not supported\n",
#else
          "         -n, --sort-by-name, -N, --natural-sort, --sort-picard, -M, --match-mates\n"
          "               not supported: coordinate order only\n",
#endif
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, SBX_SORT_PROG ": %s\n", m.c_str());
    return 1;
}

// setExtension(path, "sorted.bam"): the extension of the last path component is replaced (appended when there is none)
std::string with_sorted_extension(const std::string& path) {
    const size_t slash = path.find_last_of('/');
    const size_t dot = path.find_last_of('.');
    const size_t name0 = slash == std::string::npos ? 0 : slash + 1;
    const bool has_ext = dot != std::string::npos && dot > name0;
    return (has_ext ? path.substr(0, dot) : path) + ".sorted.bam";
}

bool ends_with(const std::string& s, const char* t) {
    const size_t n = strlen(t);
    return s.size() >= n && s.compare(s.size() - n, n, t) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::string out, filter_str, level_str;
    std::vector<std::string> files;
    bool by_name = false, natural = false, match_mates = false;
    // long name, short name, takes a value, what it does: 0 ignored, 1 out, 2 level, 3 filter, 4 refused, 5 -n, 6 -N, 7 -M
    constexpr int kN = SBX_SORT_BY_NAME ? 5 : 4, kNat = SBX_SORT_BY_NAME ? 6 : 4, kM = SBX_SORT_BY_NAME ? 7 : 4;
    static const sbx::OptSpec opts[] = {
        {"memory-limit", 'm', true, 0}, {"tmpdir", 0, true, 0}, {"out", 'o', true, 1}, {"sort-by-name", 'n', false, kN},
        {"natural-sort", 'N', false, kNat}, {"sort-picard", 0, false, 4}, {"match-mates", 'M', false, kM},
        {"uncompressed-chunks", 'u', false, 0}, {"compression-level", 'l', true, 2}, {"show-progress", 'p', false, 0},
        {"nthreads", 't', true, 0}, {"filter", 'F', true, 3},
    };
    for (int i = 1; i < argc; ++i) {
        const sbx::OptToken t = sbx::next_opt(argc, argv, &i, opts);
        if (t.kind == sbx::OptToken::Terminator) {       // `--` ends the options
            for (++i; i < argc; ++i) files.push_back(argv[i]);
            break;
        }
        if (t.kind == sbx::OptToken::Positional) { files.push_back(t.arg); continue; }
        // (bundled flags are not D getopt's default either: a short flag with text attached is no option at all)
        if (t.kind == sbx::OptToken::Unknown || (t.attached && !t.spec->takes_value && t.arg[1] != '-')) return die("Unrecognized option " + t.arg);
        const sbx::OptSpec& o = *t.spec;
        const std::string shown = o.sht ? std::string("-") + o.sht + " / --" + o.lng : std::string("--") + o.lng;
        if (o.id == 4)
            return die("option " + shown + (SBX_SORT_BY_NAME ? " is not supported" : " is not supported: sbx-sort sorts by coordinate only"));
        if (o.id == 5) { by_name = true; continue; }
        if (o.id == 6) { natural = true; continue; }
        if (o.id == 7) { match_mates = true; continue; }
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        if (o.id == 1) out = t.value;
        else if (o.id == 2) level_str = t.value;
        else if (o.id == 3) filter_str = t.value;
    }
    if (by_name && natural) return die("only one of -n and -N and -s parameters can be provided");
    if (match_mates && !(by_name || natural)) return die("-M option only works in combination with either -n or -N");
    if (files.empty()) {
        usage();
        return 1;
    }
    const std::string in = files[0];
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
    }
    if (out.empty()) out = with_sorted_extension(in);
    char err[512] = {0};
    sbx_filter filter;
    const bool have_filter = !filter_str.empty();
    if (have_filter && sbx_compile_filter(filter_str.c_str(), &filter, err, sizeof err) != SBX_OK) return die(err);
    const sbx_filter* fp = have_filter ? &filter : nullptr;
    const int rc = by_name || natural
                       ? sbx_sort_bam_by_name(in.c_str(), out.c_str(), fp, level, natural ? 2 : 1, match_mates ? 1 : 0, -1, nullptr, err, sizeof err)
                       : sbx_sort_bam(in.c_str(), out.c_str(), fp, level, ends_with(out, ".bam") ? 1 : 0, -1, nullptr, err, sizeof err);
    if (rc != SBX_OK) return die(err);
    return 0;
}
