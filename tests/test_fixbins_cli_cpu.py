"""The option policy of sbx-fixbins, pinned byte for byte in the manner of tests/test_view_cli_cpu.py: it scans its arguments with
csrc/cli_opts.hpp, accepts and ignores -t and -p, prints the usage with exit status 0 for anything but two file names (as fixbins_main
does), words a bad level as sbx-view does, and refuses an output that is the input before anything is opened.  Every vector is
decided before a device is used, or ends in the library's open; nothing is created on the way."""
import os
import subprocess

import pytest

import sambamba_amd

USAGE = (
    b"Usage: sbx-fixbins [options] <input.bam> <output.bam>\n\n"
    b"Options: -t, --nthreads=NTHREADS, -p, --show-progress\n"
    b"                    accepted for compatibility; the bins are computed on the GPU\n"
    b"         -l, --compression-level=LEVEL\n"
    b"                    specify compression level (from 0 to 9)\n")

# (arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    ([], 0, b"", USAGE),
    (["in.bam"], 0, b"", USAGE),
    (["-l", "3", "-p", "in.bam"], 0, b"", USAGE),
    (["a.bam", "b.bam", "c.bam"], 0, b"", USAGE),
    (["--"], 0, b"", USAGE),
    (["-l", "10", "a.bam", "b.bam"], 1, b"", b"sbx-fixbins: invalid compression level 10\n"),
    (["-l=x", "a.bam", "b.bam"], 1, b"", b"sbx-fixbins: invalid compression level x\n"),
    (["--compression-level", "-2", "a.bam", "b.bam"], 1, b"", b"sbx-fixbins: invalid compression level -2\n"),
    (["a.bam", "b.bam", "--compression-level=3x"], 1, b"", b"sbx-fixbins: invalid compression level 3x\n"),
    (["a.bam", "b.bam", "-l"], 1, b"", b"sbx-fixbins: Missing value for argument -l.\n"),
    (["a.bam", "b.bam", "-t"], 1, b"", b"sbx-fixbins: Missing value for argument -t.\n"),
    (["--bogus", "a.bam", "b.bam"], 1, b"", b"sbx-fixbins: Unrecognized option --bogus\n"),
    (["-c", "a.bam", "b.bam"], 1, b"", b"sbx-fixbins: Unrecognized option -c\n"),
    (["-px", "a.bam", "b.bam"], 1, b"", b"sbx-fixbins: Unrecognized option -px\n"),
]

# accepted by the options, refused by the open of the input
REACH_OPEN = [
    ["in.bam", "out.bam"],
    ["-t", "4", "-p", "-l", "0", "in.bam", "out.bam"],
    ["in.bam", "-l9", "out.bam", "--nthreads=2", "--show-progress"],
    ["--compression-level=-1", "--", "in.bam", "out.bam"],
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.fixbins_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("args,status,stdout,stderr", DECIDED, ids=[" ".join(["sbx-fixbins"] + c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, status, stdout, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", REACH_OPEN, ids=[" ".join(["sbx-fixbins"] + c) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = b"sbx-fixbins: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == b"sbx-fixbins: can't open file in.bam\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_output_equal_to_input_is_refused_first(tmp_path):
    path = tmp_path / "in.bam"
    path.write_bytes(b"not even a BAM file")
    for args in (["in.bam", "in.bam"], ["-l", "1", "in.bam", "./in.bam"], ["in.bam", str(path)]):
        r = run(args, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"sbx-fixbins: the output would overwrite the input in.bam\n")
    assert path.read_bytes() == b"not even a BAM file" and os.listdir(str(tmp_path)) == ["in.bam"]


def test_binding_names_the_binary():
    assert os.path.basename(sambamba_amd.fixbins_cli_path()) == "sbx-fixbins" and os.access(sambamba_amd.fixbins_cli_path(), os.X_OK)
