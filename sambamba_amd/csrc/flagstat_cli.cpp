// flagstat_cli.cpp -- `sbx-flagstat`: the standalone `sambamba-flagstat` (flagstat_main, sambamba/flagstat.d:82-148) on top of the
// C ABI of libsbx_depth.so.  The counting happens on the device (sbx_flagstat); this file parses the options and prints.
//
//   sbx-flagstat [-t N|--nthreads=N] [-p|--show-progress] [-b|--tabular] in.bam
//
// As with D's getopt, options may follow the file name (cli_opts.hpp scans them); `--` ends the options.  Messages carry no prefix.
// -t is validated in every spelling ("Invalid number of threads: V"); anything else that starts with `-` and is longer than one
// character is "Unrecognized option X" -- a flag with text attached (`-bx`, `--tabular=1`) included; a lone `-` is a file.  -t only sizes the reference's decompression pool and is accepted and
// ignored; so is -p (the device pass reports no progress).  The counters are printed only after the whole file was read
// (flagstat.d:127-145): on any error stdout stays empty, the message goes to stderr and the exit status is 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-flagstat [options] <input.bam>\n"
          "\n"
          "Counts the records of a BAM file by their flags, as `sambamba flagstat` does, on the GPU.\n"
          "\n"
          "Options: -t, --nthreads=N     accepted for compatibility; the GPU does the decompression\n"
          "         -p, --show-progress  accepted for compatibility; no progress is drawn\n"
          "         -b, --tabular        print comma-separated values\n",
          stderr);
}

bool parse_count(const char* s) {
    if (!s || !*s) return false;
    char* end = nullptr;
    strtoull(s, &end, 10);
    return *end == 0 && s[0] != '-';
}

}  // namespace

int main(int argc, char** argv) {
    bool tabular = false;
    std::vector<std::string> files;
    static const sbx::OptSpec opts[] = {{"nthreads", 't', true, 't'}, {"show-progress", 'p', false, 'p'}, {"tabular", 'b', false, 'b'}};
    for (int i = 1; i < argc; ++i) {
        const sbx::OptToken t = sbx::next_opt(argc, argv, &i, opts);
        if (t.kind == sbx::OptToken::Terminator) {
            for (++i; i < argc; ++i) files.push_back(argv[i]);
            break;
        }
        if (t.kind == sbx::OptToken::Positional) { files.push_back(t.arg); continue; }       // (a lone `-` as well)
        // a flag is its exact spelling: with text attached (`-bx`, `--tabular=1`) it is as unknown as `--bogus`
        if (t.kind == sbx::OptToken::Unknown || (t.attached && !t.spec->takes_value)) { fprintf(stderr, "Unrecognized option %s\n", t.arg.c_str()); return 1; }
        if (t.missing) { fprintf(stderr, "Missing value for argument %s.\n", t.arg.c_str()); return 1; }
        if (t.spec->id == 'b') tabular = true;
        else if (t.spec->id == 't' && !parse_count(t.value.c_str())) { fprintf(stderr, "Invalid number of threads: %s\n", t.value.c_str()); return 1; }
    }
    if (files.empty()) {
        usage();
        return 1;
    }
    sbx_flagstat_counts f;
    char err[512] = {0};
    if (sbx_flagstat(files[0].c_str(), -1, &f, err, sizeof err) != SBX_OK) {
        fprintf(stderr, "%s\n", err);
        return 1;
    }
    size_t n = 0;
    sbx_format_flagstat(&f, tabular ? 1 : 0, nullptr, 0, &n);
    std::vector<char> text(n + 1);
    if (sbx_format_flagstat(&f, tabular ? 1 : 0, text.data(), text.size(), &n) != SBX_OK) {
        fprintf(stderr, "cannot format the counters\n");
        return 1;
    }
    if (fwrite(text.data(), 1, n, stdout) != n || fflush(stdout) != 0) {
        fprintf(stderr, "error writing the output\n");
        return 1;
    }
    return 0;
}
