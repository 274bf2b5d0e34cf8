// view_cli.cpp -- `sbx-view`: the command line of `sambamba-view` (view_main / sambambaMain, sambamba/view.d:149-403) on top of the
// C ABI of libsbx_depth.so.  Reading, selecting and compressing happen on the device (sbx_view_run); this file parses the options
// and prints the host-only outputs (-H, -I).
//
//   sbx-view [options] <input.bam> [region1 [...]]
//
// Two sinks exist: -c (the count) and -f bam.  The other formats -- sam, which is the reference's default, json, unpack, msgpack,
// cram --, -v / --valid and -S / --sam-input are refused by name.  -t, -p and -T are accepted and ignored; -h is accepted and has no
// effect on BAM output.  As in sambambaMain, -c wins over -I and -H (and ignores -h and -f), and -I wins over -H.  As with D's getopt,
// options may follow the file name (cli_opts.hpp scans them) and `--` ends the options.  Without arguments the usage goes to stderr
// and the exit status is 0, as in the reference.  Without --subsampling-seed a random 64-bit seed is drawn.  The @PG line's CL is
// "view" followed by the arguments as given.  Errors: "sbx-view: <message>" on stderr and exit status 1.
//
// Compiled a second time with -DSBX_VIEW_SAM=1 this file is `sbx-sam`: the same options under the same policy, with the third sink
// (SBX_VIEW_SINK_SAM).  There `sam` is the default format as in the reference, -f sam and -f bam are both taken, -h writes the header in
// front of the SAM records, -l together with SAM output is refused, and -v / --valid is taken for all three sinks: only the records
// the reference's isValid accepts are selected (sbx_view_request::valid_only, K19).  (sbx-view keeps refusing sam and -v: folding the
// two into one executable is the removal of this switch.)
//
// Compiled a third time with -DSBX_VIEW_INDEXED=1 it is `sbx-iview`: sbx-sam's options and sinks, and a region or -L reads only the
// blocks the .bai names (sbx_view_run_indexed in REQUIRED mode, as the reference needs the index for a region); --no-index selects the
// whole-file pass of the other two.  --no-index is not part of the @PG line's CL: the two passes write the same bytes.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/sbx_depth.h"
#include "cli_opts.hpp"

#ifndef SBX_VIEW_INDEXED
#define SBX_VIEW_INDEXED 0
#endif
#if SBX_VIEW_INDEXED
#undef SBX_VIEW_SAM
#define SBX_VIEW_SAM 1
#endif
#ifndef SBX_VIEW_SAM
#define SBX_VIEW_SAM 0
#endif

namespace {

#if SBX_VIEW_INDEXED
const char* const kProgram = "sbx-iview";

void usage() {
    fputs("Usage: sbx-iview [options] <input.bam> [region1 [...]]\n"
          "\n"
          "Selects records of a BAM file, as `sambamba view` does, on the GPU; writes them as SAM (the default), as a BAM (-f bam)\n"
          "or their number (-c).  The SAM text is formatted on the GPU.\n"
          "\n"
          "Options: -F, --filter=FILTER\n"
          "                    set custom filter for alignments\n"
          "         --num-filter=NUMFILTER\n"
          "                    filter flag bits; 'i1/i2' corresponds to -f i1 -F i2 samtools arguments;\n"
          "                    either of the numbers can be omitted\n"
          "         -f, --format=sam|bam\n"
          "                    output format (default: sam); json, unpack, msgpack and cram are not supported\n"
          "         -h, --with-header\n"
          "                    print header before reads (always done for BAM output)\n"
          "         -H, --header\n"
          "                    output only header to stdout, as SAM\n"
          "         -I, --reference-info\n"
          "                    output to stdout only reference names and lengths in JSON\n"
          "         -L, --regions=FILENAME\n"
          "                    output only reads overlapping one of regions from the BED file\n"
          "         -c, --count\n"
          "                    output to stdout only count of matching records, hHI are ignored\n"
          "         -l, --compression-level\n"
          "                    specify compression level (from 0 to 9, works only for BAM output)\n"
          "         -o, --output-filename\n"
          "                    specify output filename (default, and '-': stdout)\n"
          "         -s, --subsample=FRACTION\n"
          "                    subsample reads (read pairs)\n"
          "         --subsampling-seed=SEED\n"
          "                    set seed for subsampling\n"
          "         -v, --valid\n"
          "                    output only valid alignments\n"
          "         -t, --nthreads=NTHREADS, -p, --show-progress, -T, --ref-filename=FASTA\n"
          "                    accepted for compatibility\n"
          "         --no-index\n"
          "                    read the whole file even for a region or -L (no .bai needed)\n"
          "         -S, --sam-input\n"
          "                    not supported\n"
          "\n"
          "Regions are 'chr', 'chr:beg-end' or '*' (reads without a reference); at most 1024 may be listed, a BED file has no limit.\n"
          "A read that overlaps several listed regions is written once per region.  With a region or -L only the blocks the .bai names\n"
          "are read, and the .bai is required; without either, or with --no-index, the whole file is read.\n",
          stderr);
}
#elif SBX_VIEW_SAM
const char* const kProgram = "sbx-sam";

void usage() {
    fputs("Usage: sbx-sam [options] <input.bam> [region1 [...]]\n"
          "\n"
          "Selects records of a BAM file, as `sambamba view` does, on the GPU; writes them as SAM (the default), as a BAM (-f bam)\n"
          "or their number (-c).  The SAM text is formatted on the GPU.\n"
          "\n"
          "Options: -F, --filter=FILTER\n"
          "                    set custom filter for alignments\n"
          "         --num-filter=NUMFILTER\n"
          "                    filter flag bits; 'i1/i2' corresponds to -f i1 -F i2 samtools arguments;\n"
          "                    either of the numbers can be omitted\n"
          "         -f, --format=sam|bam\n"
          "                    output format (default: sam); json, unpack, msgpack and cram are not supported\n"
          "         -h, --with-header\n"
          "                    print header before reads (always done for BAM output)\n"
          "         -H, --header\n"
          "                    output only header to stdout, as SAM\n"
          "         -I, --reference-info\n"
          "                    output to stdout only reference names and lengths in JSON\n"
          "         -L, --regions=FILENAME\n"
          "                    output only reads overlapping one of regions from the BED file\n"
          "         -c, --count\n"
          "                    output to stdout only count of matching records, hHI are ignored\n"
          "         -l, --compression-level\n"
          "                    specify compression level (from 0 to 9, works only for BAM output)\n"
          "         -o, --output-filename\n"
          "                    specify output filename (default, and '-': stdout)\n"
          "         -s, --subsample=FRACTION\n"
          "                    subsample reads (read pairs)\n"
          "         --subsampling-seed=SEED\n"
          "                    set seed for subsampling\n"
          "         -v, --valid\n"
          "                    output only valid alignments\n"
          "         -t, --nthreads=NTHREADS, -p, --show-progress, -T, --ref-filename=FASTA\n"
          "                    accepted for compatibility\n"
          "         -S, --sam-input\n"
          "                    not supported\n"
          "\n"
          "Regions are 'chr', 'chr:beg-end' or '*' (reads without a reference); at most 1024 may be listed, a BED file has no limit.\n"
          "A read that overlaps several listed regions is written once per region.  No index is needed; the whole file is read.\n",
          stderr);
}
#else
const char* const kProgram = "sbx-view";

void usage() {
    fputs("Usage: sbx-view [options] <input.bam> [region1 [...]]\n"
          "\n"
          "Selects records of a BAM file, as `sambamba view` does, on the GPU; writes a BAM (-f bam) or their number (-c).\n"
          "\n"
          "Options: -F, --filter=FILTER\n"
          "                    set custom filter for alignments\n"
          "         --num-filter=NUMFILTER\n"
          "                    filter flag bits; 'i1/i2' corresponds to -f i1 -F i2 samtools arguments;\n"
          "                    either of the numbers can be omitted\n"
          "         -f, --format=bam\n"
          "                    output format; only bam is supported (sam, the reference's default, json, unpack,\n"
          "                    msgpack and cram are not): give -f bam or -c\n"
          "         -h, --with-header\n"
          "                    accepted; the header is always written for BAM output\n"
          "         -H, --header\n"
          "                    output only header to stdout, as SAM\n"
          "         -I, --reference-info\n"
          "                    output to stdout only reference names and lengths in JSON\n"
          "         -L, --regions=FILENAME\n"
          "                    output only reads overlapping one of regions from the BED file\n"
          "         -c, --count\n"
          "                    output to stdout only count of matching records, hHI are ignored\n"
          "         -l, --compression-level\n"
          "                    specify compression level (from 0 to 9)\n"
          "         -o, --output-filename\n"
          "                    specify output filename (default, and '-': stdout)\n"
          "         -s, --subsample=FRACTION\n"
          "                    subsample reads (read pairs)\n"
          "         --subsampling-seed=SEED\n"
          "                    set seed for subsampling\n"
          "         -t, --nthreads=NTHREADS, -p, --show-progress, -T, --ref-filename=FASTA\n"
          "                    accepted for compatibility\n"
          "         -v, --valid, -S, --sam-input\n"
          "                    not supported\n"
          "\n"
          "Regions are 'chr', 'chr:beg-end' or '*' (reads without a reference); at most 1024 may be listed, a BED file has no limit.\n"
          "A read that overlaps several listed regions is written once per region.  No index is needed; the whole file is read.\n",
          stderr);
}
#endif

int die(const std::string& m) {
    fprintf(stderr, "%s: %s\n", kProgram, m.c_str());
    return 1;
}

// the text of a host-only output of an open file, to stdout
int print_text(const std::string& in, bool reference_info) {
    char err[512] = {0};
    const char* one[1] = {in.c_str()};
    sbx_ctx* c = sbx_open(one, 1, -1, err, sizeof err);
    if (!c) return die(err);
    std::string out;
    size_t n = 0;
    int rc;
    if (reference_info) {
        sbx_view_reference_info(c, nullptr, 0, &n);
        out.assign(n + 1, '\0');
        rc = sbx_view_reference_info(c, &out[0], out.size(), &n);
    } else {
        // HeaderSerializer(stdout, format).writeln(header) before addPG: toSam of the parsed text, no @PG added (view.d:248-253)
        size_t tn = 0;
        const char* t = sbx_header_text(c, &tn);
        const std::string text(t ? t : "", t ? tn : 0);
        sbx_markdup_header_text(text.data(), text.size(), nullptr, nullptr, 0, &n);
        out.assign(n + 1, '\0');
        rc = sbx_markdup_header_text(text.data(), text.size(), nullptr, &out[0], out.size(), &n);
    }
    sbx_close(c);
    if (rc != SBX_OK) return die(reference_info ? "cannot list the references" : "malformed SAM header text");
    out.resize(n);
    fwrite(out.data(), 1, out.size(), stdout);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    std::string filter_str, num_filter, format = "sam", bed, level_str, out, frac_str, seed_str;
    bool have_num_filter = false, have_frac = false, have_seed = false, header_only = false, reference_info = false, count_only = false, with_header = false, valid_only = false, no_index = false;
    std::vector<std::string> files;
    // long name, short name, takes a value, what it does: 0 ignored, 1 filter, 2 num-filter, 3 format, 4 -H, 5 -I, 6 -L, 7 -c, 8 level, 9 out,
    // 10 fraction, 11 seed, 12 refused, 13 -h, 14 -v, 15 --no-index
    static const sbx::OptSpec opts[] = {
        {"filter", 'F', true, 1}, {"num-filter", 0, true, 2}, {"format", 'f', true, 3}, {"with-header", 'h', false, 13}, {"header", 'H', false, 4},
        {"reference-info", 'I', false, 5}, {"regions", 'L', true, 6}, {"count", 'c', false, 7}, {"valid", 'v', false, SBX_VIEW_SAM ? 14 : 12},
        {"sam-input", 'S', false, 12}, {"show-progress", 'p', false, 0}, {"compression-level", 'l', true, 8}, {"output-filename", 'o', true, 9},
        {"nthreads", 't', true, 0}, {"subsample", 's', true, 10}, {"subsampling-seed", 0, true, 11}, {"ref-filename", 'T', true, 0},
#if SBX_VIEW_INDEXED
        {"no-index", 0, false, 15},
#endif
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
        if (o.id == 12) return die(std::string("option -") + o.sht + " / --" + o.lng + " is not supported");
        if (t.missing) return die("Missing value for argument " + t.arg + ".");
        switch (o.id) {
            case 1: filter_str = t.value; break;
            case 2: num_filter = t.value; have_num_filter = true; break;
            case 3: format = t.value; break;
            case 4: header_only = true; break;
            case 5: reference_info = true; break;
            case 6: bed = t.value; break;
            case 7: count_only = true; break;
            case 8: level_str = t.value; break;
            case 9: out = t.value; break;
            case 10: frac_str = t.value; have_frac = true; break;
            case 11: seed_str = t.value; have_seed = true; break;
            case 13: with_header = true; break;
            case 14: valid_only = true; break;
            case 15: no_index = true; break;
            default: break;
        }
    }
    if (files.empty()) {
        usage();
        return 0;
    }
    const std::string in = files[0];
    if (reference_info && !count_only) return print_text(in, true);
    if (header_only && !count_only) return print_text(in, false);
    const bool sam_out = SBX_VIEW_SAM && !count_only && format == "sam";
    if (!count_only && format != "bam" && !sam_out) {
        if (format == "sam" || format == "json" || format == "unpack" || format == "msgpack" || format == "cram")
            return die("output format " + format + " is not supported yet: use -f bam or -c");
        return die("output format must be one of sam, bam, json");                        // view.d:397
    }
    int level = -1;
    if (!level_str.empty()) {
        char* end = nullptr;
        const long v = strtol(level_str.c_str(), &end, 10);
        if (*end || v < -1 || v > 9) return die("invalid compression level " + level_str);
        level = (int)v;
        if (sam_out) return die("-l / --compression-level applies to BAM output only: give -f bam");
    }
    sbx_view_opts vo;
    memset(&vo, 0, sizeof vo);
    if (have_num_filter && sbx_view_num_filter(num_filter.c_str(), &vo.flags_set, &vo.flags_unset) != SBX_OK)
        return die("invalid --num-filter " + num_filter + ": expected i1/i2, two numbers from 0 to 65535, either of which may be missing");
    if (have_frac) {
        char* end = nullptr;
        const double f = strtod(frac_str.c_str(), &end);
        if (frac_str.empty() || *end || std::isnan(f) || f < 0) return die("invalid subsampling fraction " + frac_str);
        vo.subsample = 1;
        vo.fraction = f;
        if (have_seed) {
            char* e2 = nullptr;
            const unsigned long long v = strtoull(seed_str.c_str(), &e2, 10);
            if (seed_str.empty() || seed_str[0] == '-' || *e2) return die("invalid subsampling seed " + seed_str);
            vo.seed = v;
        } else {
            std::random_device rd;                         // unpredictableSeed, twice (view.d:160-162)
            vo.seed = ((uint64_t)rd() << 32) + rd();
        }
    }
    if (!bed.empty() && files.size() > 1) return die("specifying both region and BED filename is disallowed");
    if (files.size() - 1 > SBX_VIEW_MAX_REGIONS)
        return die("too many regions (" + std::to_string(files.size() - 1) + "): at most " + std::to_string(SBX_VIEW_MAX_REGIONS) +
                   " may be listed; use -L with a BED file");
    char err[512] = {0};
    sbx_filter filter;
    const bool have_filter = !filter_str.empty();
    if (have_filter && sbx_compile_filter(filter_str.c_str(), &filter, err, sizeof err) != SBX_OK) return die(err);
    std::vector<const char*> regions;
    for (size_t k = 1; k < files.size(); ++k) regions.push_back(files[k].c_str());
    sbx_view_request q;
    memset(&q, 0, sizeof q);
    q.struct_size = (uint32_t)sizeof q;
    q.in_path = in.c_str();
    q.filter = have_filter ? &filter : nullptr;
    q.opts = &vo;
    q.regions = regions.data();
    q.n_regions = regions.size();
    q.bed_path = bed.c_str();
    q.level = level;
    q.device = -1;
    q.valid_only = valid_only ? 1 : 0;
    // sbx-iview: the read pass follows the index unless --no-index
    auto run = [&](const sbx_view_request* request, uint64_t* count, char* e, size_t n) {
#if SBX_VIEW_INDEXED
        return sbx_view_run_indexed(request, no_index ? SBX_VIEW_INDEX_OFF : SBX_VIEW_INDEX_REQUIRED, count, nullptr, nullptr, e, n);
#else
        (void)no_index;
        return sbx_view_run(request, count, nullptr, e, n);
#endif
    };
    if (count_only) {
        uint64_t count = 0;
        q.sink = SBX_VIEW_SINK_COUNT;
        if (run(&q, &count, err, sizeof err) != SBX_OK) return die(err);
        printf("%llu\n", (unsigned long long)count);
        return 0;
    }
    std::string cl = "view";
    for (int i = 1; i < argc; ++i) {
        if (SBX_VIEW_INDEXED && !strcmp(argv[i], "--no-index")) continue;
        cl += ' ';
        cl += argv[i];
    }
    q.sink = sam_out ? SBX_VIEW_SINK_SAM : SBX_VIEW_SINK_BAM;
    q.out_path = out.empty() ? "-" : out.c_str();
    q.pg_command_line = cl.c_str();
    q.with_header = with_header ? 1 : 0;
    if (run(&q, nullptr, err, sizeof err) != SBX_OK) return die(err);
    return 0;
}
