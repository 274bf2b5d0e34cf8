// validate_cli.cpp -- `sbx-validate`: the command `sambamba validate` names ("simple validator (BAM)") and leaves empty
// (validate_main, sambamba/validate.d), on top of the C ABI of libsbx_depth.so.  The records are judged on the device
// (sbx_validate_bam, K19); this file parses the options and prints.
//
//   sbx-validate [-t N|--nthreads=N] [-p|--show-progress] <input.bam> [<input2.bam> ...]
//
// Per file, on stdout, the tab-separated lines of sbx_format_validate_report: file, records, invalid, the ten classes of error with
// the number of records in each (a record can be in several), and for a file with invalid records the first of them in file order.
// The exit status is 0 when every file is clean and 1 otherwise.  Without a file the usage goes to stderr and the status is 1, as
// validate_main's.  -t and -p are accepted and ignored.  As with D's getopt, options may follow the file names (cli_opts.hpp scans
// them) and `--` ends the options.  Errors: "sbx-validate: <message>" on stderr and exit status 1; the files in front have been
// reported by then.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-validate [options] <input.bam> [<input2.bam> [...]]\n"
          "\n"
          "Checks every record of the BAM files, as `sambamba view --valid` judges them, on the GPU; prints per file the number of\n"
          "records, of invalid records, of records per class of error, and the first invalid record.\n"
          "The exit status is 0 when every record of every file is valid.\n"
          "\n"
          "Options: -t, --nthreads=N     accepted for compatibility; the GPU does the decompression\n"
          "         -p, --show-progress  accepted for compatibility; no progress is drawn\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-validate: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::string> files;
    static const sbx::OptSpec opts[] = {{"nthreads", 't', true, 't'}, {"show-progress", 'p', false, 'p'}};
    for (int i = 1; i < argc; ++i) {
        const sbx::OptToken t = sbx::next_opt(argc, argv, &i, opts);
        if (t.kind == sbx::OptToken::Terminator) {
            for (++i; i < argc; ++i) files.push_back(argv[i]);
            break;
        }
        if (t.kind == sbx::OptToken::Positional) { files.push_back(t.arg); continue; }
        if (t.kind == sbx::OptToken::Unknown || (t.attached && !t.spec->takes_value)) return die("Unrecognized option " + t.arg);
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
    }
    if (files.empty()) {
        usage();
        return 1;
    }
    bool clean = true;
    for (const std::string& f : files) {
        sbx_validate_report r;
        char err[512] = {0};
        if (sbx_validate_bam(f.c_str(), -1, &r, nullptr, err, sizeof err) != SBX_OK) return die(err);
        size_t n = 0;
        sbx_format_validate_report(f.c_str(), &r, nullptr, 0, &n);
        std::vector<char> text(n + 1);
        if (sbx_format_validate_report(f.c_str(), &r, text.data(), text.size(), &n) != SBX_OK) return die("cannot format the report");
        if (fwrite(text.data(), 1, n, stdout) != n || fflush(stdout) != 0) return die("error writing the output");
        clean = clean && r.n_invalid == 0;
    }
    return clean ? 0 : 1;
}
