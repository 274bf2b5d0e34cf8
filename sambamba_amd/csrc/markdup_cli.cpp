// markdup_cli.cpp -- `sbx-markdup`: the command line of `sambamba-markdup` (markdup_main, sambamba/markdup.d:1130-1317) on top of the
// C ABI of libsbx_depth.so.  Reading, finding the duplicates and compressing happen on the device (sbx_markdup); this file parses the
// options and prints the reference's messages.
//
//   sbx-markdup [-r|--remove-duplicates] [-l N|--compression-level=N] <input.bam> <output.bam>
//
// -t, -p, --tmpdir, --hash-table-size, --overflow-list-size, --sort-buffer-size and --io-buffer-size are accepted and ignored: the
// file is resident in device memory, there is no hash table, no temporary file and no thread pool.  --compare-with-picard-mode (a
// development aid of the reference) is refused by name, and so is more than one input (the reference merges their headers).  As with
// D's getopt, options may follow the file names (cli_opts.hpp scans them) and `--` ends the options.  With fewer than two file names
// the usage goes to stderr and the exit status is 0, as in the reference.  The @PG line's CL is "markdup" followed by the arguments
// as given.  Errors: "sbx-markdup: <message>" on stderr and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sys/stat.h>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-markdup [options] <input.bam> <output.bam>\n"
          "       By default, marks the duplicates without removing them\n"
          "\n"
          "Options: -r, --remove-duplicates\n"
          "                    remove duplicates instead of just marking them\n"
          "         -l, --compression-level=N\n"
          "                    specify compression level of the resulting file (from 0 to 9)\n"
          "         -t, --nthreads=NTHREADS, -p, --show-progress, --tmpdir=TMPDIR, --hash-table-size=N, --overflow-list-size=N,\n"
          "         --sort-buffer-size=N, --io-buffer-size=N\n"
          "                    accepted for compatibility; the duplicates are found in GPU memory\n"
          "         --compare-with-picard-mode, more than one input file\n"
          "                    not supported\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-markdup: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    std::string level_str;
    std::vector<std::string> files;
    bool remove = false;
    // long name, short name, takes a value, what it does: 0 ignored, 1 remove, 2 level, 4 refused
    static const sbx::OptSpec opts[] = {
        {"remove-duplicates", 'r', false, 1}, {"nthreads", 't', true, 0}, {"compression-level", 'l', true, 2}, {"show-progress", 'p', false, 0},
        {"tmpdir", 0, true, 0}, {"hash-table-size", 0, true, 0}, {"overflow-list-size", 0, true, 0}, {"io-buffer-size", 0, true, 0},
        {"sort-buffer-size", 0, true, 0}, {"compare-with-picard-mode", 0, false, 4},
    };
    for (int i = 1; i < argc; ++i) {
        const sbx::OptToken t = sbx::next_opt(argc, argv, &i, opts);
        if (t.kind == sbx::OptToken::Terminator) {       // `--` ends the options
            for (++i; i < argc; ++i) files.push_back(argv[i]);
            break;
        }
        if (t.kind == sbx::OptToken::Positional) { files.push_back(t.arg); continue; }
        if (t.kind == sbx::OptToken::Unknown || (t.attached && !t.spec->takes_value && t.arg[1] != '-')) return die("Unrecognized option " + t.arg);
        const sbx::OptSpec& o = *t.spec;
        if (o.id == 4) return die(std::string("option --") + o.lng + " is not supported");
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        if (o.id == 1) remove = true;
        else if (o.id == 2) level_str = t.value;
    }
    if (files.size() < 2) {
        usage();
        return 0;
    }
    if (files.size() > 2) return die("more than one input file is not supported: sbx-markdup does not merge headers");
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
    }
    std::string cl = "markdup";
    for (int i = 1; i < argc; ++i) { cl += ' '; cl += argv[i]; }
    // protectFromOverwrite comes before the first message in the reference too
    struct stat sa, sb;
    if (stat(files[0].c_str(), &sa) == 0 && stat(files[1].c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino)
        return die("the output would overwrite the input " + files[0]);
    char err[512] = {0};
    fputs("finding positions of the duplicate reads in the file...\n", stderr);
    sbx_markdup_stats st;
    const int rc = sbx_markdup(files[0].c_str(), files[1].c_str(), remove ? 1 : 0, level, cl.c_str(), -1, &st, err, sizeof err);
    if (rc != SBX_OK) return die(err);
    fprintf(stderr, "  sorted %llu end pairs\n", (unsigned long long)st.n_end_pairs);
    fprintf(stderr, "     and %llu single ends (among them %llu unmatched pairs)\n", (unsigned long long)st.n_single_ends,
            (unsigned long long)st.n_unmatched_pairs);
    fprintf(stderr, "  found %llu duplicates\n", (unsigned long long)st.n_duplicates);
    fputs(remove ? "removing duplicates...\n" : "marking duplicates...\n", stderr);
    return 0;
}
