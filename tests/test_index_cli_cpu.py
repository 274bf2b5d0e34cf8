"""The option policy of sbx-index, pinned byte for byte in the manner of tests/test_view_cli_cpu.py: it scans its arguments with
csrc/cli_opts.hpp, accepts and ignores -t and -p, prints the usage with exit status 0 for anything but one or two file names (as
index_main does), and prints the reference's two lines before it indexes a FASTA file.  Every vector is decided before a device is
used, or ends in the library's open; nothing is created on the way."""
import os
import subprocess

import pytest

import sambamba_amd

USAGE = (
    b"Usage: sbx-index [OPTIONS] <input.bam|input.fasta> [output_file]\n\n"
    b"\tCreates index for a BAM, or FASTA file\n\n"
    b"Options: -t, --nthreads=NTHREADS, -p, --show-progress\n"
    b"               accepted for compatibility; the index is built on the GPU\n"
    b"         -c, --check-bins\n"
    b"               check that bins are set correctly\n"
    b"         -F, --fasta-input\n"
    b"               specify that input is in FASTA format\n")
INDEXING = b"Indexing FASTA file...\n"
NO_BAR = b"[info] progressbar is unavailable for FASTA input\n"

# (arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    ([], 0, b"", USAGE),
    (["-c"], 0, b"", USAGE),
    (["-F", "-p", "-t", "3"], 0, b"", USAGE),
    (["a.bam", "b.bai", "c"], 0, b"", USAGE),
    (["--"], 0, b"", USAGE),
    (["--", "a", "b", "c"], 0, b"", USAGE),
    (["in.bam", "-t"], 1, b"", b"sbx-index: Missing value for argument -t.\n"),
    (["--nthreads"], 1, b"", b"sbx-index: Missing value for argument --nthreads.\n"),
    (["--bogus", "in.bam"], 1, b"", b"sbx-index: Unrecognized option --bogus\n"),
    (["-x", "in.bam"], 1, b"", b"sbx-index: Unrecognized option -x\n"),
    (["-cF", "in.bam"], 1, b"", b"sbx-index: Unrecognized option -cF\n"),
    (["-l", "3", "in.bam"], 1, b"", b"sbx-index: Unrecognized option -l\n"),
]

# accepted by the options, refused by the open of the input: (arguments, what stderr starts with, the open's message)
REACH_OPEN = [
    (["in.bam"], b"", b"can't open file in.bam"),
    (["in.bam", "out.bai"], b"", b"can't open file in.bam"),
    (["-c", "in.bam"], b"", b"can't open file in.bam"),
    (["in.bam", "--check-bins", "-t", "4", "-p", "out.bai"], b"", b"can't open file in.bam"),
    (["-t4", "--nthreads=2", "--show-progress", "--", "in.bam"], b"", b"can't open file in.bam"),
    (["-F", "in.fasta"], INDEXING, b"cannot read in.fasta"),
    (["in.fasta", "out.fai", "--fasta-input", "-p"], INDEXING + NO_BAR, b"cannot read in.fasta"),
    (["-F", "-c", "in.fasta"], INDEXING, b"cannot read in.fasta"),
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.index_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("args,status,stdout,stderr", DECIDED, ids=[" ".join(["sbx-index"] + c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, status, stdout, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args,head,message", REACH_OPEN, ids=[" ".join(["sbx-index"] + c[0]) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args, head, message):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = head + b"sbx-index: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == head + b"sbx-index: " + message + b"\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == head.count(b"\n") + 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_binding_names_the_binary():
    assert os.path.basename(sambamba_amd.index_cli_path()) == "sbx-index" and os.access(sambamba_amd.index_cli_path(), os.X_OK)
