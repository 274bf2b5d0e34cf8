"""The option policy of sbx-slice, pinned byte for byte in the manner of tests/test_view_cli_cpu.py: it scans its arguments with
csrc/cli_opts.hpp, refuses -F / --fasta-input by name, prints the reference's messages for a missing selection and for -L next to a
region, and prints the usage with exit status 0 when it has no file name (as slice_main does).  Every vector is decided before a
device is used, or ends in the library's open."""
import os
import subprocess

import pytest

import sambamba_amd

USAGE = (
    b"Usage: sbx-slice [options] <input.bam> [region1 [...]]\n"
    b"\n"
    b"Copies regions of an indexed BAM file to a new one, as `sambamba slice` does: only the BGZF blocks around the two\n"
    b"edges of a region are read and compressed again (on the GPU), every block in between is copied as it is.\n"
    b"\n"
    b"Options: -o, --output-filename=OUTPUT_FILENAME\n"
    b"                    output BAM filename (default, and '-': stdout)\n"
    b"         -L, --regions=FILENAME\n"
    b"                    copy the regions of the BED file (merged, in reference order) instead of listed ones\n"
    b"         -F, --fasta-input\n"
    b"                    not supported\n"
    b"\n"
    b"Regions are 'chr', 'chr:beg' or 'chr:beg-end'; at most 1024 may be listed, a BED file has no limit.  '*' alone copies\n"
    b"the reads without a reference.  Regions that overlap give their common reads twice.  The input needs its .bai.\n")

FASTA = b"sbx-slice: option -F / --fasta-input is not supported\n"
NEITHER = b"sbx-slice: Must provide either a bed file or list of regions.\n"
BOTH = b"sbx-slice: specifying both region and BED filename is disallowed\n"

# (arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    ([], 0, b"", USAGE),
    (["-o", "out.bam"], 0, b"", USAGE),
    (["-L", "r.bed"], 0, b"", USAGE),
    (["--"], 0, b"", USAGE),
    (["-F", "in.fa", "chr1"], 1, b"", FASTA),
    (["in.fa", "chr1", "--fasta-input"], 1, b"", FASTA),
    (["-F", "-L", "r.bed", "in.fa"], 1, b"", FASTA),                      # (-L with FASTA: -F is refused first)
    (["in.bam"], 1, b"", NEITHER),
    (["-o", "out.bam", "in.bam"], 1, b"", NEITHER),
    (["--", "in.bam"], 1, b"", NEITHER),
    (["-L", "", "in.bam"], 1, b"", NEITHER),
    (["-L", "r.bed", "in.bam", "chr1"], 1, b"", BOTH),
    (["in.bam", "chr1:1-10", "*", "--regions=r.bed"], 1, b"", BOTH),
    (["in.bam", "chr1", "-o"], 1, b"", b"sbx-slice: Missing value for argument -o.\n"),
    (["in.bam", "--regions"], 1, b"", b"sbx-slice: Missing value for argument --regions.\n"),
    (["--bogus", "in.bam", "chr1"], 1, b"", b"sbx-slice: Unrecognized option --bogus\n"),
    (["-Fx", "in.bam", "chr1"], 1, b"", b"sbx-slice: Unrecognized option -Fx\n"),
    (["-l", "3", "in.bam", "chr1"], 1, b"", b"sbx-slice: Unrecognized option -l\n"),
    (["in.bam"] + ["chr1:%d-%d" % (k + 1, k + 10) for k in range(1025)], 1, b"",
     b"sbx-slice: too many regions (1025): at most 1024 may be listed; use -L with a BED file\n"),
]

# accepted by the options, refused by the open of the input
REACH_OPEN = [
    ["in.bam", "chr1"],
    ["in.bam", "*"],
    ["-o", "out.bam", "in.bam", "chr1:100-200", "chr2"],
    ["--output-filename=out.bam", "in.bam", "chr1:100"],
    ["-oout.bam", "in.bam", "chr1"],
    ["-L", "r.bed", "in.bam"],
    ["in.bam", "--regions=r.bed", "-o", "-"],
    ["--", "in.bam", "chr1"],
    ["in.bam"] + ["chr1:%d-%d" % (k + 1, k + 10) for k in range(1024)],
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.slice_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


def _id(args):
    s = " ".join(["sbx-slice"] + args)
    return s if len(s) < 80 else s[:60] + "...(%d arguments)" % len(args)


@pytest.mark.parametrize("args,status,stdout,stderr", DECIDED, ids=[_id(c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, status, stdout, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", REACH_OPEN, ids=[_id(c) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = b"sbx-slice: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == b"sbx-slice: can't open file in.bam\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_output_equal_to_input_is_refused(tmp_path):
    path = tmp_path / "in.bam"
    path.write_bytes(b"not even a BAM file")
    r = run(["-o", str(path), str(path), "chr1"], tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    assert r.stderr == b"sbx-slice: the output would overwrite the input " + str(path).encode() + b"\n"
    assert path.read_bytes() == b"not even a BAM file"
