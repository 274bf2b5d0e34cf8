// subsample_cli.cpp -- `sbx-subsample`: the command line of `sambamba subsample` (subsample_main, sambamba/subsample.d:336-463) on top
// of the C ABI of libsbx_depth.so.  Reading, the coverage, the verdicts and compressing happen on the device (sbx_subsample); this
// file parses the options.
//
//   sbx-subsample --type fasthash --max-cov N -o <output.bam> [-r] [-l LEVEL] <input.bam>
//
// As with D's getopt, options may follow the file name (cli_opts.hpp scans them) and `--` ends the options.  Without any argument
// the usage goes to stdout and the exit status is 1, as in the reference.  The refusals come in the reference's order and words:
// "Output not defined", "Algorithm not defined", "Maximum coverage not set" (a value <= 0 too), "Input file can not be same as
// output file <name>".  More than one input is refused by name: the reference would overwrite the one output once per input.
// --logging is accepted and ignored.  -l is an addition (the reference hard-codes level 9): -1, the default, or 0 .. 9.  The @PG
// line's CL is "subsample" followed by the arguments as given.  Errors: "sbx-subsample: <message>" on stderr and exit status 1.
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
    fputs("\n"
          "Usage: sbx-subsample [options] <input.bam>\n"
          "\n"
          "       Subsample a bam file.\n"
          "\n"
          "Options:\n"
          "\n"
          "         --type [fasthash]   Algorithm for subsampling (fasthash, default is none)\n"
          "         --max-cov [depth]   Maximum coverage (approx)\n"
          "         -o, --output fn     Set output file\n"
          "         -r, --remove        Remove over sampled reads from output\n"
          "                             (default: mark them as failing quality control, flag 0x200)\n"
          "         -l level            Compression level of the output (0 to 9, default -1: the encoder's)\n"
          "\n"
          "         --logging type      accepted for compatibility\n"
          "\n"
          "Examples:\n"
          "\n"
          "       sbx-subsample --type=fasthash --max-cov=50 input.bam -ooutput.bam\n"
          "\n",
          stdout);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-subsample: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        usage();
        return 1;
    }
    std::string type, max_cov_str, output, level_str;
    std::vector<std::string> files;
    bool remove = false;
    // long name, short name, takes a value, what it does: 0 ignored, 1 type, 2 max-cov, 3 output, 4 remove, 5 level
    static const sbx::OptSpec opts[] = {
        {"type", 0, true, 1}, {"max-cov", 0, true, 2}, {"output", 'o', true, 3}, {"remove", 'r', false, 4},
        {"compression-level", 'l', true, 5}, {"logging", 0, true, 0},
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
        switch (t.spec->id) {
            case 1: type = t.value; break;
            case 2: max_cov_str = t.value; break;
            case 3: output = t.value; break;
            case 4: remove = true; break;
            case 5: level_str = t.value; break;
            default: break;
        }
    }
    int max_cov = 0;
    if (!max_cov_str.empty()) {
        char* end = nullptr;
        const long v = strtol(max_cov_str.c_str(), &end, 10);
        if (*end || v < -2147483647L - 1 || v > 2147483647L) return die("invalid maximum coverage " + max_cov_str);
        max_cov = (int)v;
    }
    // the reference's enforce() calls, in its order
    if (output.empty()) return die("Output not defined");
    if (type != "fasthash") return die("Algorithm not defined");
    if (max_cov <= 0) return die("Maximum coverage not set");
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
    }
    if (files.empty()) return die("no input file");
    if (files.size() > 1)
        return die("more than one input file is not supported: " + output + " would be overwritten once per input (" + files[0] + ", " + files[1] +
                   (files.size() > 2 ? ", ..." : "") + ")");
    struct stat sa, sb;
    if (output == files[0] ||
        (stat(files[0].c_str(), &sa) == 0 && stat(output.c_str(), &sb) == 0 && sa.st_dev == sb.st_dev && sa.st_ino == sb.st_ino))
        return die("Input file can not be same as output file " + files[0]);
    std::string cl = "subsample";
    for (int i = 1; i < argc; ++i) { cl += ' '; cl += argv[i]; }
    char err[1024] = {0};
    const int rc = sbx_subsample(files[0].c_str(), output.c_str(), max_cov, remove ? 1 : 0, level, 0, cl.c_str(), -1, nullptr, nullptr, err,
                                 sizeof err);
    if (rc != SBX_OK) return die(err);
    return 0;
}
