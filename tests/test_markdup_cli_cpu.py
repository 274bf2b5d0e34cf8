"""The option policy of sbx-markdup, pinned byte for byte in the manner of tests/test_cli_options_cpu.py: it scans its arguments with
csrc/cli_opts.hpp, accepts and ignores the reference's tuning options, refuses --compare-with-picard-mode and a second input by name,
prints the usage with exit status 0 when it has fewer than two file names (as markdup_main does), and refuses an output that is the
input before it prints anything else.  Every vector is decided before a device is used, or ends in the library's open."""
import os
import subprocess

import pytest

import sambamba_amd

USAGE = (
    b"Usage: sbx-markdup [options] <input.bam> <output.bam>\n"
    b"       By default, marks the duplicates without removing them\n\n"
    b"Options: -r, --remove-duplicates\n"
    b"                    remove duplicates instead of just marking them\n"
    b"         -l, --compression-level=N\n"
    b"                    specify compression level of the resulting file (from 0 to 9)\n"
    b"         -t, --nthreads=NTHREADS, -p, --show-progress, --tmpdir=TMPDIR, --hash-table-size=N, --overflow-list-size=N,\n"
    b"         --sort-buffer-size=N, --io-buffer-size=N\n"
    b"                    accepted for compatibility; the duplicates are found in GPU memory\n"
    b"         --compare-with-picard-mode, more than one input file\n"
    b"                    not supported\n")
FINDING = b"finding positions of the duplicate reads in the file...\n"

# (arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    ([], 0, b"", USAGE),
    (["in.bam"], 0, b"", USAGE),
    (["-r", "-t", "4", "in.bam"], 0, b"", USAGE),
    (["--"], 0, b"", USAGE),
    (["--compare-with-picard-mode", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: option --compare-with-picard-mode is not supported\n"),
    (["a.bam", "b.bam", "--compare-with-picard-mode"], 1, b"", b"sbx-markdup: option --compare-with-picard-mode is not supported\n"),
    (["a.bam", "b.bam", "out.bam"], 1, b"", b"sbx-markdup: more than one input file is not supported: sbx-markdup does not merge headers\n"),
    (["-l", "10", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: invalid compression level 10\n"),
    (["-l=x", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: invalid compression level x\n"),
    (["--compression-level", "-2", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: invalid compression level -2\n"),
    (["a.bam", "b.bam", "-l"], 1, b"", b"sbx-markdup: Missing value for argument -l.\n"),
    (["a.bam", "b.bam", "--tmpdir"], 1, b"", b"sbx-markdup: Missing value for argument --tmpdir.\n"),
    (["--bogus", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: Unrecognized option --bogus\n"),
    (["-x", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: Unrecognized option -x\n"),
    (["-rx", "a.bam", "b.bam"], 1, b"", b"sbx-markdup: Unrecognized option -rx\n"),
]

# accepted by the options, refused by the open of the input
REACH_OPEN = [
    ["in.bam", "out.bam"],
    ["-r", "in.bam", "out.bam"],
    ["-t", "4", "-p", "--tmpdir=/tmp", "--hash-table-size", "1000", "--overflow-list-size=7", "--sort-buffer-size=100", "--io-buffer-size", "5",
     "in.bam", "out.bam"],
    ["in.bam", "-l", "1", "out.bam", "--remove-duplicates", "--nthreads=2", "--show-progress"],
    ["--compression-level=0", "--", "in.bam", "out.bam"],
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.markdup_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("args,status,stdout,stderr", DECIDED, ids=[" ".join(["sbx-markdup"] + c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, status, stdout, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", REACH_OPEN, ids=[" ".join(["sbx-markdup"] + c) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = FINDING + b"sbx-markdup: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == FINDING + b"sbx-markdup: can't open file in.bam\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 2)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_output_equal_to_input_is_refused_first(tmp_path):
    path = tmp_path / "in.bam"
    path.write_bytes(b"not even a BAM file")
    for args in (["in.bam", "in.bam"], ["-r", "in.bam", "./in.bam"], ["in.bam", str(path)]):
        r = run(args, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"sbx-markdup: the output would overwrite the input in.bam\n")
    assert path.read_bytes() == b"not even a BAM file" and os.listdir(str(tmp_path)) == ["in.bam"]
