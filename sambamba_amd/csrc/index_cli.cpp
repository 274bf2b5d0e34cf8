// index_cli.cpp -- `sbx-index`: the command line of `sambamba-index` (index_main, sambamba/index.d:52-139) on top of the C ABI of
// libsbx_depth.so.  Reading and indexing happen on the device (sbx_index_bam, sbx_index_fasta); this file parses the options.
//
//   sbx-index [-t N] [-p] [-c] [-F] <input.bam|input.fasta> [output_file]
//
// -t and -p are accepted and ignored: there is no thread pool and no progress bar.  -c checks the bins of the placed records while
// the index is built; -F indexes a FASTA file (the reference's two messages on stderr included).  The default output is the input's
// name + ".bai" or ".fai".  As with D's getopt, options may follow the file names (cli_opts.hpp scans them) and `--` ends the options.
// With anything but one or two file names the usage goes to stderr and the exit status is 0, as in the reference.
// Errors: "sbx-index: <message>" on stderr and exit status 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-index [OPTIONS] <input.bam|input.fasta> [output_file]\n"
          "\n"
          "\tCreates index for a BAM, or FASTA file\n"
          "\n"
          "Options: -t, --nthreads=NTHREADS, -p, --show-progress\n"
          "               accepted for compatibility; the index is built on the GPU\n"
          "         -c, --check-bins\n"
          "               check that bins are set correctly\n"
          "         -F, --fasta-input\n"
          "               specify that input is in FASTA format\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-index: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    std::vector<std::string> files;
    bool check_bins = false, fasta = false, progress = false;
    // long name, short name, takes a value, what it does: 0 ignored, 1 check bins, 2 FASTA, 3 progress
    static const sbx::OptSpec opts[] = {
        {"nthreads", 't', true, 0}, {"show-progress", 'p', false, 3}, {"check-bins", 'c', false, 1}, {"fasta-input", 'F', false, 2},
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
        const int id = t.spec->id;
        if (id == 1) check_bins = true;
        else if (id == 2) fasta = true;
        else if (id == 3) progress = true;
    }
    if (files.size() != 1 && files.size() != 2) {
        usage();
        return 0;
    }
    const std::string out = files.size() > 1 ? files[1] : files[0] + (fasta ? ".fai" : ".bai");
    char err[1024] = {0};
    int rc;
    if (fasta) {
        fputs("Indexing FASTA file...\n", stderr);
        if (progress) fputs("[info] progressbar is unavailable for FASTA input\n", stderr);
        rc = sbx_index_fasta(files[0].c_str(), out.c_str(), -1, nullptr, err, sizeof err);
    } else {
        rc = sbx_index_bam(files[0].c_str(), out.c_str(), check_bins ? 1 : 0, -1, err, sizeof err);
    }
    if (rc != SBX_OK) return die(err);
    return 0;
}
