// import_cli.cpp -- `sbx-import`: `sambamba view -S -f bam` (view_main / sambambaMain with a SamReader, sambamba/view.d:216-218,
// 292-311) on top of the C ABI of libsbx_depth.so.  Reading the text is the host's, parsing the lines and compressing the BAM
// happen on the device (sbx_import_sam); this file parses the options.
//
//   sbx-import [-S] [-f bam] [-o out.bam] [-l level] [-h] [-t N] [-p] in.sam|-
//
// -S and -f bam are what the command does and may be given; -h, -t and -p are accepted and ignored (a BAM always carries its
// header).  The output goes to stdout without -o or with `-o -`.  The other formats and everything that selects records -- -F,
// --num-filter, -s, -L, -c, -v -- are refused by name: selection over imported records is not built.  A positional argument behind
// the file gets the reference's own message and exit status (view.d:293-296).  As with D's getopt, options may follow the file name
// (cli_opts.hpp scans them) and `--` ends the options.  Without arguments the usage goes to stderr and the exit status is 0, as in
// the reference.  The @PG line's CL is "view" followed by the arguments as given.  Errors: "sbx-import: <message>" on stderr and
// exit status 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-import [-S] [-f bam] [-o out.bam] [-l level] [-h] [-t N] [-p] <input.sam>|-\n"
          "\n"
          "Turns SAM text into a BAM file, as `sambamba view -S -f bam` does; the lines are parsed and the BAM is compressed on the GPU.\n"
          "\n"
          "Options: -S, --sam-input\n"
          "                    the input is SAM (implied)\n"
          "         -f, --format=bam\n"
          "                    output format (implied; sam, json, msgpack, unpack and cram are not supported)\n"
          "         -o, --output-filename\n"
          "                    specify output filename (default, and '-': stdout)\n"
          "         -l, --compression-level\n"
          "                    specify compression level (from 0 to 9)\n"
          "         -h, --with-header, -t, --nthreads=NTHREADS, -p, --show-progress\n"
          "                    accepted for compatibility\n"
          "         -F, --filter, --num-filter, -s, --subsample, -L, --regions, -c, --count, -v, --valid\n"
          "                    not supported: records of SAM input are not selected\n"
          "\n"
          "The input is a file or '-' (stdin) and is read front to back.  A line that is not a SAM alignment line ends the command\n"
          "with an error that names how many such lines there are and the first of them; no output file is left behind.\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-import: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    std::string format = "bam", level_str, out;
    std::vector<std::string> files;
    // long name, short name, takes a value, what it does: 0 ignored, 1 format, 2 level, 3 out, 4 refused
    static const sbx::OptSpec opts[] = {
        {"sam-input", 'S', false, 0}, {"format", 'f', true, 1}, {"with-header", 'h', false, 0}, {"show-progress", 'p', false, 0},
        {"nthreads", 't', true, 0}, {"compression-level", 'l', true, 2}, {"output-filename", 'o', true, 3},
        {"filter", 'F', true, 4}, {"num-filter", 0, true, 4}, {"subsample", 's', true, 4}, {"regions", 'L', true, 4},
        {"count", 'c', false, 4}, {"valid", 'v', false, 4},
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
        if (o.id == 4)
            return die((o.sht ? std::string("option -") + o.sht + " / --" + o.lng : std::string("option --") + o.lng) +
                       " is not supported: records of SAM input are not selected");
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        switch (o.id) {
            case 1: format = t.value; break;
            case 2: level_str = t.value; break;
            case 3: out = t.value; break;
            default: break;
        }
    }
    if (files.empty()) {
        usage();
        return 0;
    }
    if (format != "bam") {
        if (format == "sam" || format == "json" || format == "msgpack" || format == "unpack" || format == "cram")
            return die("output format " + format + " is not supported: sbx-import writes BAM (-f bam)");
        return die("output format must be one of sam, bam, json");                        // view.d:397
    }
    if (files.size() > 1) {                                    // view.d:293-296, message and status
        fputs("region queries are unavailable for SAM input\n", stderr);
        return 1;
    }
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
    }
    std::string cl = "view";
    for (int i = 1; i < argc; ++i) { cl += ' '; cl += argv[i]; }
    char err[512] = {0};
    const int rc = sbx_import_sam(files[0].c_str(), out.empty() ? "-" : out.c_str(), cl.c_str(), level, 0, -1, nullptr, err, sizeof err);
    if (rc != SBX_OK) return die(err);
    return 0;
}
