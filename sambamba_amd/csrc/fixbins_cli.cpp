// fixbins_cli.cpp -- `sbx-fixbins`: the command line of `sambamba-fixbins` (fixbins_main, sambamba/fixbins.d:45-99) on top of the C ABI
// of libsbx_depth.so.  Reading, the bins and compressing happen on the device (sbx_fixbins); this file parses the options.
//
//   sbx-fixbins [-t N] [-p] [-l LEVEL] <input.bam> <output.bam>
//
// -t and -p are accepted and ignored.  As with D's getopt, options may follow the file names (cli_opts.hpp scans them) and `--` ends
// the options.  With anything but two file names the usage goes to stderr and the exit status is 0, as in the reference.  An output
// that is the input is refused before anything is opened (protectFromOverwrite comes first in the reference too).
// Errors: "sbx-fixbins: <message>" on stderr and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <sys/stat.h>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-fixbins [options] <input.bam> <output.bam>\n"
          "\n"
          "Options: -t, --nthreads=NTHREADS, -p, --show-progress\n"
          "                    accepted for compatibility; the bins are computed on the GPU\n"
          "         -l, --compression-level=LEVEL\n"
          "                    specify compression level (from 0 to 9)\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-fixbins: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    std::string level_str;
    std::vector<std::string> files;
    // long name, short name, takes a value, what it does: 0 ignored, 2 level
    static const sbx::OptSpec opts[] = {
        {"nthreads", 't', true, 0}, {"show-progress", 'p', false, 0}, {"compression-level", 'l', true, 2},
    };
    for (int i = 1; i < argc; ++i) {
        const sbx::OptToken t = sbx::next_opt(argc, argv, &i, opts);
        if (t.kind == sbx::OptToken::Terminator) {       // `--` ends the options
            for (++i; i < argc; ++i) files.push_back(argv[i]);
            break;
        }
        if (t.kind == sbx::OptToken::Positional) { files.push_back(t.arg); continue; }
        if (t.kind == sbx::OptToken::Unknown || (t.attached && !t.spec->takes_value && t.arg[1] != '-')) return die("Unrecognized option " + t.arg);
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        if (t.spec->id == 2) level_str = t.value;
    }
    if (files.size() != 2) {
        usage();
        return 0;
    }
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
    }
    struct stat sa, sb;
    if (stat(files[0].c_str(), &sa) == 0 && stat(files[1].c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino)
        return die("the output would overwrite the input " + files[0]);
    char err[1024] = {0};
    const int rc = sbx_fixbins(files[0].c_str(), files[1].c_str(), level, -1, nullptr, err, sizeof err);
    if (rc != SBX_OK) return die(err);
    return 0;
}
