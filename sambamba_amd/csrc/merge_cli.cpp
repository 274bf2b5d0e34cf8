// merge_cli.cpp -- `sbx-merge`: the command line of `sambamba-merge` (merge_main, sambamba/merge.d:300-420) on top of the C ABI of
// libsbx_depth.so.  Reading, rewriting, merging and compressing happen on the device (sbx_merge_bam); this file parses the options.
//
//   sbx-merge [-l N|--compression-level=N] [-F FILTER|--filter=FILTER] [-H|--header] <output.bam> <input1.bam> <input2.bam> [...]
//
// -H writes the merged header text to stdout and no file.  -t, -p and -v / --validate-headers are accepted and ignored: there is no
// thread pool and no progress bar, and a header the parser accepts is merged.  As with D's getopt, options may follow the file names
// (cli_opts.hpp scans them) and `--` ends the options.  With fewer than three file names the usage goes to stderr and the exit status
// is 1, as in the reference.  Like the reference's BamWriter, an output whose name ends in ".bam" gets a "<out>.bai" next to it.
// Errors: "sbx-merge: <message>" on stderr and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-merge [options] <output.bam> <input1.bam> <input2.bam> [...]\n"
          "\n"
          "Merges coordinate-sorted BAM files into one, as `sambamba merge` does, on the GPU.\n"
          "\n"
          "Options: -l, --compression-level=COMPRESSION_LEVEL\n"
          "               level of compression for merged BAM file, number from 0 to 9\n"
          "         -H, --header\n"
          "               output merged header to stdout in SAM format, other options are ignored; mainly for debug purposes\n"
          "         -F, --filter=FILTER\n"
          "               keep only reads that satisfy FILTER\n"
          "         -t, --nthreads=NTHREADS, -p, --show-progress, -v, --validate-headers\n"
          "               accepted for compatibility\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-merge: %s\n", m.c_str());
    return 1;
}

bool ends_with(const std::string& s, const char* t) {
    const size_t n = strlen(t);
    return s.size() >= n && s.compare(s.size() - n, n, t) == 0;
}

bool has_sq_line(const std::string& text) {
    return text.compare(0, 4, "@SQ\t") == 0 || text.find("\n@SQ\t") != std::string::npos;
}

// The merged header of the inputs, to stdout.  One input is open at a time: its text is copied and the context closed.  A text
// without @SQ lines gets them from the binary reference list, as sbx_merge_bam does, so that -H prints the header the file would get.
// (sbx_open is the only reader of a BAM header the C ABI has, and it needs a device.)
int print_header(const std::vector<std::string>& inputs) {
    std::vector<std::string> held;
    char err[512] = {0};
    for (const std::string& path : inputs) {
        const char* one[1] = {path.c_str()};
        sbx_ctx* c = sbx_open(one, 1, -1, err, sizeof err);
        if (!c) return die(err);
        size_t n = 0;
        const char* t = sbx_header_text(c, &n);
        std::string text(t ? t : "", t ? n : 0);
        sbx_header_info hi;
        if (sbx_header(c, &hi) == SBX_OK && hi.n_ref > 0 && !has_sq_line(text)) {
            if (!text.empty() && text.back() != '\n') text += '\n';
            for (int r = 0; r < hi.n_ref; ++r) text += std::string("@SQ\tSN:") + sbx_ref_name(c, r) + "\tLN:" + std::to_string(sbx_ref_length(c, r)) + "\n";
        }
        sbx_close(c);
        held.push_back(text);
    }
    std::vector<const char*> texts;
    std::vector<size_t> lens;
    for (const std::string& t : held) { texts.push_back(t.data()); lens.push_back(t.size()); }
    size_t n = 0;
    sbx_merge_header_text(texts.data(), lens.data(), (int)texts.size(), nullptr, 0, &n);
    std::string out(n + 1, '\0');
    const int code = sbx_merge_header_text(texts.data(), lens.data(), (int)texts.size(), &out[0], out.size(), &n);
    out.resize(n);
    if (code != SBX_OK) return die(out);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::string filter_str, level_str;
    std::vector<std::string> files;
    bool header_only = false;
    // long name, short name, takes a value, what it does: 0 ignored, 1 header, 2 level, 3 filter
    static const sbx::OptSpec opts[] = {
        {"nthreads", 't', true, 0}, {"compression-level", 'l', true, 2}, {"validate-headers", 'v', false, 0}, {"header", 'H', false, 1},
        {"show-progress", 'p', false, 0}, {"filter", 'F', true, 3},
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
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        if (o.id == 1) header_only = true;
        else if (o.id == 2) level_str = t.value;
        else if (o.id == 3) filter_str = t.value;
    }
    if (files.size() < 3) {
        usage();
        return 1;
    }
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
    }
    char err[512] = {0};
    sbx_filter filter;
    const bool have_filter = !filter_str.empty();
    if (have_filter && sbx_compile_filter(filter_str.c_str(), &filter, err, sizeof err) != SBX_OK) return die(err);
    const std::string out = files[0];
    const std::vector<std::string> inputs(files.begin() + 1, files.end());
    if (header_only) return print_header(inputs);
    std::vector<const char*> paths;
    for (const std::string& p : inputs) paths.push_back(p.c_str());
    const int rc = sbx_merge_bam(out.c_str(), paths.data(), (int)paths.size(), have_filter ? &filter : nullptr, level, ends_with(out, ".bam") ? 1 : 0, -1,
                                 nullptr, err, sizeof err);
    if (rc != SBX_OK) return die(err);
    return 0;
}
