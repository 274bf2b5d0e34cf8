// slice_cli.cpp -- `sbx-slice`: the command line of `sambamba-slice` (slice_main, sambamba/slice.d:291-380) on top of the C ABI of
// libsbx_depth.so.  Edge runs, K18, the compressed pieces and the splice writer are sbx_slice_bam; this file parses the options.
//
//   sbx-slice [-o out.bam] [-L file.bed] <input.bam> [region1 [...]]
//
// -F / --fasta-input (the .fai fetch has no device work) is refused by name.  As with D's getopt, options may follow the file name
// (cli_opts.hpp scans them) and `--` ends the options.  Without a file argument the usage goes to stderr and the exit status is 0, as
// in the reference.  Errors: "sbx-slice: <message>" on stderr and exit status 1; three of the messages are the reference's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

namespace {

void usage() {
    fputs("Usage: sbx-slice [options] <input.bam> [region1 [...]]\n"
          "\n"
          "Copies regions of an indexed BAM file to a new one, as `sambamba slice` does: only the BGZF blocks around the two\n"
          "edges of a region are read and compressed again (on the GPU), every block in between is copied as it is.\n"
          "\n"
          "Options: -o, --output-filename=OUTPUT_FILENAME\n"
          "                    output BAM filename (default, and '-': stdout)\n"
          "         -L, --regions=FILENAME\n"
          "                    copy the regions of the BED file (merged, in reference order) instead of listed ones\n"
          "         -F, --fasta-input\n"
          "                    not supported\n"
          "\n"
          "Regions are 'chr', 'chr:beg' or 'chr:beg-end'; at most 1024 may be listed, a BED file has no limit.  '*' alone copies\n"
          "the reads without a reference.  Regions that overlap give their common reads twice.  The input needs its .bai.\n",
          stderr);
}

int die(const std::string& m) {
    fprintf(stderr, "sbx-slice: %s\n", m.c_str());
    return 1;
}

}  // namespace

int main(int argc, char** argv) {
    std::string out, bed;
    bool have_bed = false;
    std::vector<std::string> files;
    // what an option does: 1 output, 2 BED file, 3 refused
    static const sbx::OptSpec opts[] = {{"output-filename", 'o', true, 1}, {"regions", 'L', true, 2}, {"fasta-input", 'F', false, 3}};
    for (int i = 1; i < argc; ++i) {
        const sbx::OptToken t = sbx::next_opt(argc, argv, &i, opts);
        if (t.kind == sbx::OptToken::Terminator) {       // `--` ends the options
            for (++i; i < argc; ++i) files.push_back(argv[i]);
            break;
        }
        if (t.kind == sbx::OptToken::Positional) { files.push_back(t.arg); continue; }
        if (t.kind == sbx::OptToken::Unknown || (t.attached && !t.spec->takes_value && t.arg[1] != '-')) return die("Unrecognized option " + t.arg);
        const sbx::OptSpec& o = *t.spec;
        if (o.id == 3) return die(std::string("option -") + o.sht + " / --" + o.lng + " is not supported");
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        if (o.id == 1) out = t.value;
        else { bed = t.value; have_bed = true; }
    }
    if (files.empty()) {
        usage();
        return 0;
    }
    if (!have_bed && files.size() < 2) return die("Must provide either a bed file or list of regions.");                 // slice.d:316-318
    if (!bed.empty() && files.size() > 1) return die("specifying both region and BED filename is disallowed");           // slice.d:321-323
    if (have_bed && bed.empty() && files.size() < 2) return die("Must provide either a bed file or list of regions.");
    if (files.size() - 1 > SBX_VIEW_MAX_REGIONS)
        return die("too many regions (" + std::to_string(files.size() - 1) + "): at most " + std::to_string(SBX_VIEW_MAX_REGIONS) +
                   " may be listed; use -L with a BED file");
    std::vector<const char*> regions;
    for (size_t k = 1; k < files.size(); ++k) regions.push_back(files[k].c_str());
    char err[512] = {0};
    const int rc = sbx_slice_bam(files[0].c_str(), out.empty() ? "-" : out.c_str(), regions.data(), regions.size(), bed.c_str(), -1, nullptr, err,
                                 sizeof err);
    if (rc != SBX_OK) return die(err);
    return 0;
}
