"""The option policies of the three command lines (sbx-depth, sbx-sort, sbx-flagstat), pinned byte for byte.

All three scan their arguments with csrc/cli_opts.hpp; what they DO with a token differs, and the differences are the contract:
sbx-depth turns what it does not know into a file name and never validates a number (D getopt with passThrough), sbx-sort
refuses by name and ends the options at `--`, sbx-flagstat prints no prefix and validates -t.  Every argument vector below is
decided before a device is used; the expected exit status, stdout and stderr were recorded from the binaries as they were before
the scanners were merged and are literals, not derived from the code under test.

A vector that gets past the options ends in the library's open.  Without a device that fails with "no HIP device available",
with one it fails on the file that does not exist -- `reached` names the argument that must have become the input file."""
import os
import subprocess

import pytest

import sambamba_amd

D, S, F = "sbx-depth", "sbx-sort", "sbx-flagstat"
BIN = {D: sambamba_amd.cli_path, S: sambamba_amd.sort_cli_path, F: sambamba_amd.flagstat_cli_path}

DEPTH_USAGE = (
    b"Usage: sambamba-depth region|window|base [options] input.bam  [input2.bam [...]]\n\n"
    b"          All BAM files must be coordinate-sorted and indexed.\n\n"
    b"          The tool has three modes: base, region, and window,\n"
    b"          each name means per which unit to print the statistics.\n\n"
    b"Common options:\n"
    b"         -F, --filter=FILTER\n"
    b"                    set custom filter for alignments; the default value is\n"
    b"                    'mapping_quality > 0 and not duplicate and not failed_quality_control'\n"
    b"         -o, --output-file=FILENAME\n"
    b"                    output filename (by default /dev/stdout)\n"
    b"         -t, --nthreads=NTHREADS\n"
    b"                    maximum number of threads to use\n"
    b"         -c, --min-coverage=MINCOVERAGE\n"
    b"                    minimum mean coverage for output (default: 0 for region/window, 1 for base)\n"
    b"         -C, --max-coverage=MAXCOVERAGE\n"
    b"                    maximum mean coverage for output\n"
    b"         -q, --min-base-quality=QUAL\n"
    b"                    don't count bases with lower base quality\n"
    b"         --combined\n"
    b"                    output combined statistics for all samples\n"
    b"         -a, --annotate\n"
    b"                    add additional column of y/n instead of\n"
    b"                    skipping records not satisfying the criteria\n"
    b"         -m, --fix-mate-overlaps\n"
    b"                    detect overlaps of mate reads and handle them on per-base basis\n"
    b"base subcommand options:\n"
    b"         -L, --regions=FILENAME|REGION\n"
    b"                    list or regions of interest or a single region in form chr:beg-end (optional)\n"
    b"         -z, --report-zero-coverage (DEPRECATED, use --min-coverage=0 instead)\n"
    b"                    don't skip zero coverage bases\n"
    b"region subcommand options:\n"
    b"         -L, --regions=FILENAME|REGION\n"
    b"                    list or regions of interest or a single region in form chr:beg-end (required)\n"
    b"         -T, --cov-threshold=COVTHRESHOLD\n"
    b"                    multiple thresholds can be provided,\n"
    b"                    for each one an extra column will be added,\n"
    b"                    the percentage of bases in the region\n"
    b"                    where coverage is more than this value\n"
    b"window subcommand options:\n"
    b"         -w, --window-size=WINDOWSIZE\n"
    b"                    breadth of the window, in bp (required)\n"
    b"         --overlap=OVERLAP\n"
    b"                    overlap of successive windows, in bp (default is 0)\n"
    b"         -T, --cov-threshold=COVTHRESHOLD\n"
    b"                    same meaning as in 'region' subcommand\n")

SORT_USAGE = (
    b"Usage: sbx-sort [options] <input.bam>\n\n"
    b"Sorts a BAM file by coordinate, as `sambamba sort` does, on the GPU.\n\n"
    b"Options: -o, --out=OUTPUTFILE\n"
    b"               output file name; if not provided, the result is written to a file with .sorted.bam extension\n"
    b"         -l, --compression-level=COMPRESSION_LEVEL\n"
    b"               level of compression for sorted BAM, from 0 to 9\n"
    b"         -F, --filter=FILTER\n"
    b"               keep only reads that satisfy FILTER\n"
    b"         -m, --memory-limit=LIMIT, --tmpdir=TMPDIR, -u, --uncompressed-chunks, -t, --nthreads=NTHREADS, -p, --show-progress\n"
    b"               accepted for compatibility; the file is sorted in GPU memory\n"
    b"         -n, --sort-by-name, -N, --natural-sort, --sort-picard, -M, --match-mates\n"
    b"               not supported: coordinate order only\n")

FLAGSTAT_USAGE = (
    b"Usage: sbx-flagstat [options] <input.bam>\n\n"
    b"Counts the records of a BAM file by their flags, as `sambamba flagstat` does, on the GPU.\n\n"
    b"Options: -t, --nthreads=N     accepted for compatibility; the GPU does the decompression\n"
    b"         -p, --show-progress  accepted for compatibility; no progress is drawn\n"
    b"         -b, --tabular        print comma-separated values\n")

BAD_FILTER = (b"filter: 'nonsense((' is outside the device-compilable subset (flags, integer fields, integer tags, tag existence, "
              b"and/or/not)\n")
BASE_HEADER = b"REF\tPOS\tCOV\tA\tC\tG\tT\tDEL\tREFSKIP"

# (binary, arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    # ---- sbx-depth: every spelling of a value, before and after the file name
    (D, ["base", "--filter=nonsense((", "x.bam"], 1, b"", b"sambamba-depth: " + BAD_FILTER),
    (D, ["base", "--filter", "nonsense((", "x.bam"], 1, b"", b"sambamba-depth: " + BAD_FILTER),
    (D, ["base", "-Fnonsense((", "x.bam"], 1, b"", b"sambamba-depth: " + BAD_FILTER),
    (D, ["base", "-F=nonsense((", "x.bam"], 1, b"", b"sambamba-depth: " + BAD_FILTER),
    (D, ["base", "-F", "nonsense((", "x.bam"], 1, b"", b"sambamba-depth: " + BAD_FILTER),
    (D, ["base", "x.bam", "-F", "nonsense(("], 1, b"", b"sambamba-depth: " + BAD_FILTER),
    # a value-taking option in the last place
    (D, ["base", "-F"], 1, b"", b"sambamba-depth: Missing value for argument -F.\n"),
    (D, ["base", "x.bam", "--filter"], 1, b"", b"sambamba-depth: Missing value for argument --filter.\n"),
    (D, ["window", "x.bam", "-w"], 1, b"", b"sambamba-depth: Missing value for argument -w.\n"),
    (D, ["region", "-L"], 1, b"", b"sambamba-depth: Missing value for argument -L.\n"),
    # validation of the modes; numbers go through strtoull unvalidated ("abc" is 0)
    (D, ["region", "x.bam"], 1, b"", b"BED file or a region must be provided in region mode\n"),
    (D, ["window", "x.bam"], 1, b"", b"sambamba-depth: positive window size must be specified\n"),
    (D, ["window", "--window-size=abc", "x.bam"], 1, b"", b"sambamba-depth: positive window size must be specified\n"),
    (D, ["window", "-w", "10", "--overlap", "10", "x.bam"], 1, b"", b"sambamba-depth: specified overlap is larger than window size\n"),
    (D, ["window", "-w10", "--overlap=11", "x.bam"], 1, b"", b"sambamba-depth: specified overlap is larger than window size\n"),
    (D, ["base", "-o", "no-such-dir/out.txt", "x.bam"], 1, b"",
     b"sambamba-depth: Cannot open file `no-such-dir/out.txt' in mode `w+' (No such file or directory)\n"),
    (D, ["base", "-a"], 1, b"", b"sambamba-depth: no input files\n"),
    # usage, exit status 0: too few arguments, an unknown mode (an option in the mode's place included)
    (D, [], 0, b"", DEPTH_USAGE),
    (D, ["base"], 0, b"", DEPTH_USAGE),
    (D, ["pileup", "x.bam"], 0, b"", DEPTH_USAGE),
    (D, ["--filter", "x.bam"], 0, b"", DEPTH_USAGE),
    # ---- sbx-sort: the orders it does not sort in are refused by name, short or long, with or without `=`
    (S, ["-n", "in.bam"], 1, b"", b"sbx-sort: option -n / --sort-by-name is not supported: sbx-sort sorts by coordinate only\n"),
    (S, ["-N", "in.bam"], 1, b"", b"sbx-sort: option -N / --natural-sort is not supported: sbx-sort sorts by coordinate only\n"),
    (S, ["--sort-picard", "in.bam"], 1, b"", b"sbx-sort: option --sort-picard is not supported: sbx-sort sorts by coordinate only\n"),
    (S, ["-M", "in.bam"], 1, b"", b"sbx-sort: option -M / --match-mates is not supported: sbx-sort sorts by coordinate only\n"),
    (S, ["--sort-by-name", "in.bam"], 1, b"", b"sbx-sort: option -n / --sort-by-name is not supported: sbx-sort sorts by coordinate only\n"),
    (S, ["--natural-sort=1", "in.bam"], 1, b"", b"sbx-sort: option -N / --natural-sort is not supported: sbx-sort sorts by coordinate only\n"),
    (S, ["in.bam", "--match-mates"], 1, b"", b"sbx-sort: option -M / --match-mates is not supported: sbx-sort sorts by coordinate only\n"),
    # the compression level, in every spelling
    (S, ["-l", "10", "in.bam"], 1, b"", b"sbx-sort: invalid compression level 10\n"),
    (S, ["-l10", "in.bam"], 1, b"", b"sbx-sort: invalid compression level 10\n"),
    (S, ["-l=x", "in.bam"], 1, b"", b"sbx-sort: invalid compression level x\n"),
    (S, ["--compression-level=10", "in.bam"], 1, b"", b"sbx-sort: invalid compression level 10\n"),
    (S, ["--compression-level", "-2", "in.bam"], 1, b"", b"sbx-sort: invalid compression level -2\n"),
    (S, ["in.bam", "-l"], 1, b"", b"sbx-sort: Missing value for argument -l.\n"),
    (S, ["in.bam", "--out"], 1, b"", b"sbx-sort: Missing value for argument --out.\n"),
    # unknown options; a short flag with text attached is unknown as well
    (S, ["--bogus", "in.bam"], 1, b"", b"sbx-sort: Unrecognized option --bogus\n"),
    (S, ["-x", "in.bam"], 1, b"", b"sbx-sort: Unrecognized option -x\n"),
    (S, ["-ux", "in.bam"], 1, b"", b"sbx-sort: Unrecognized option -ux\n"),
    (S, ["-nx", "in.bam"], 1, b"", b"sbx-sort: Unrecognized option -nx\n"),
    (S, ["--filter=nonsense((", "in.bam"], 1, b"", b"sbx-sort: " + BAD_FILTER),
    (S, ["--filter", "nonsense((", "in.bam"], 1, b"", b"sbx-sort: " + BAD_FILTER),
    (S, ["-Fnonsense((", "in.bam"], 1, b"", b"sbx-sort: " + BAD_FILTER),
    (S, ["-F=nonsense((", "in.bam"], 1, b"", b"sbx-sort: " + BAD_FILTER),
    (S, ["-F", "nonsense((", "in.bam"], 1, b"", b"sbx-sort: " + BAD_FILTER),
    (S, ["in.bam", "-F", "nonsense(("], 1, b"", b"sbx-sort: " + BAD_FILTER),
    # no file: usage, exit status 1
    (S, [], 1, b"", SORT_USAGE),
    (S, ["-u", "-p"], 1, b"", SORT_USAGE),
    (S, ["--"], 1, b"", SORT_USAGE),
    # ---- sbx-flagstat: no prefix; -t is validated in every spelling
    (F, ["in.bam", "-t"], 1, b"", b"Missing value for argument -t.\n"),
    (F, ["--nthreads"], 1, b"", b"Missing value for argument --nthreads.\n"),
    (F, ["-t", "x", "in.bam"], 1, b"", b"Invalid number of threads: x\n"),
    (F, ["-tx", "in.bam"], 1, b"", b"Invalid number of threads: x\n"),
    (F, ["-t=x", "in.bam"], 1, b"", b"Invalid number of threads: x\n"),
    (F, ["--nthreads=-1", "in.bam"], 1, b"", b"Invalid number of threads: -1\n"),
    (F, ["--nthreads", "-1", "in.bam"], 1, b"", b"Invalid number of threads: -1\n"),
    (F, ["--nthreads=", "in.bam"], 1, b"", b"Invalid number of threads: \n"),
    (F, ["-t", "", "in.bam"], 1, b"", b"Invalid number of threads: \n"),
    # anything else that starts with `-` and is longer than one character is unrecognized: flags with text attached included
    (F, ["-bx", "in.bam"], 1, b"", b"Unrecognized option -bx\n"),
    (F, ["--tabular=1", "in.bam"], 1, b"", b"Unrecognized option --tabular=1\n"),
    (F, ["-px", "in.bam"], 1, b"", b"Unrecognized option -px\n"),
    (F, ["--bogus", "in.bam"], 1, b"", b"Unrecognized option --bogus\n"),
    (F, ["-x"], 1, b"", b"Unrecognized option -x\n"),
    (F, ["in.bam", "--nthreadsx"], 1, b"", b"Unrecognized option --nthreadsx\n"),
    (F, [], 1, b"", FLAGSTAT_USAGE),
    (F, ["-b", "-p", "-t", "2"], 1, b"", FLAGSTAT_USAGE),
    (F, ["--"], 1, b"", FLAGSTAT_USAGE),
]

# (binary, arguments, stdout, prefix of the error line, the argument that became the input file): accepted by the options, refused
# by the open.  sbx-depth prints the header line of `base` and `window` before it opens the file: the columns show which flags were set.
REACH_OPEN = [
    # what sbx-depth does not know is a file name: an unknown long or short option, a bare `--`
    (D, ["base", "--no-such-option", "x.bam"], BASE_HEADER + b"\tSAMPLE\n", b"sambamba-depth: ", "--no-such-option"),
    (D, ["base", "-x", "x.bam"], BASE_HEADER + b"\tSAMPLE\n", b"sambamba-depth: ", "-x"),
    (D, ["base", "--", "x.bam"], BASE_HEADER + b"\tSAMPLE\n", b"sambamba-depth: ", "--"),
    # a flag with text attached is still that flag
    (D, ["base", "-afoo", "/nonexistent.bam"], BASE_HEADER + b"\tSAMPLE\tFLAG\n", b"sambamba-depth: ", "/nonexistent.bam"),
    (D, ["base", "--annotate=1", "--combined", "/nonexistent.bam"], BASE_HEADER + b"\tFLAG\n", b"sambamba-depth: ", "/nonexistent.bam"),
    (D, ["base", "-a", "-z", "-m", "-c", "3", "-C=9", "-q5", "-t", "2", "--gpus=1", "/nonexistent.bam"], BASE_HEADER + b"\tSAMPLE\tFLAG\n",
     b"sambamba-depth: ", "/nonexistent.bam"),
    # -L is dropped in window mode (no "must be provided", no region lookup); -T in three spellings
    (D, ["window", "-w", "10", "--overlap=3", "-L", "chr1", "-T", "5", "-T=7", "x.bam"],
     b"# chrom\tchromStart\tchromEnd\treadCount\tmeanCoverage\tpercentage5\tpercentage7\tsampleName\n", b"sambamba-depth: ", "x.bam"),
    (D, ["region", "-L", "chr1:1-2", "-T", "3", "x.bam"], b"", b"sambamba-depth: ", "x.bam"),
    # sbx-sort: `--` ends the options; the compatibility options are accepted and ignored
    (S, ["--", "-n"], b"", b"sbx-sort: ", "-n"),
    (S, ["-u", "-p", "-t", "4", "-m", "1G", "--tmpdir=/tmp", "--uncompressed-chunks=1", "-l", "3", "-o", "out.bam", "in.bam"], b"",
     b"sbx-sort: ", "in.bam"),
    # sbx-flagstat
    (F, ["-t4", "-t=4", "-t", "4", "--nthreads=4", "--nthreads", "4", "-b", "-p", "--tabular", "--show-progress", "in.bam"], b"", b"", "in.bam"),
    (F, ["--", "-b"], b"", b"", "-b"),
    (F, ["-", "-b"], b"", b"", "-"),
]


def run(exe, args, cwd):
    return subprocess.run([BIN[exe]()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=120)


@pytest.mark.parametrize("exe,args,status,stdout,stderr", DECIDED, ids=[" ".join([c[0]] + c[1]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, exe, args, status, stdout, stderr):
    r = run(exe, args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)


@pytest.mark.parametrize("exe,args,stdout,prefix,reached", REACH_OPEN, ids=[" ".join([c[0]] + c[1]) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, exe, args, stdout, prefix, reached):
    r = run(exe, args, tmp_path)
    assert (r.returncode, r.stdout) == (1, stdout)
    no_device = prefix + b"no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == prefix + b"can't open file " + reached.encode() + b"\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way
