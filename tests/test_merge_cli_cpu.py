"""The option policy of sbx-merge, pinned byte for byte in the manner of tests/test_markdup_cli_cpu.py: it scans its arguments with
csrc/cli_opts.hpp, accepts and ignores -t, -p and -v, prints the usage with exit status 1 when it has fewer than three file names (as
merge_main does), and validates the compression level and the filter before it opens a file.  Every vector is decided before a device
is used, or ends in the library's open."""
import os
import subprocess

import pytest

import sambamba_amd

USAGE = (
    b"Usage: sbx-merge [options] <output.bam> <input1.bam> <input2.bam> [...]\n\n"
    b"Merges coordinate-sorted BAM files into one, as `sambamba merge` does, on the GPU.\n\n"
    b"Options: -l, --compression-level=COMPRESSION_LEVEL\n"
    b"               level of compression for merged BAM file, number from 0 to 9\n"
    b"         -H, --header\n"
    b"               output merged header to stdout in SAM format, other options are ignored; mainly for debug purposes\n"
    b"         -F, --filter=FILTER\n"
    b"               keep only reads that satisfy FILTER\n"
    b"         -t, --nthreads=NTHREADS, -p, --show-progress, -v, --validate-headers\n"
    b"               accepted for compatibility\n")

# (arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    ([], 1, b"", USAGE),
    (["out.bam"], 1, b"", USAGE),
    (["out.bam", "a.bam"], 1, b"", USAGE),
    (["-t", "4", "-H", "out.bam", "a.bam"], 1, b"", USAGE),
    (["--"], 1, b"", USAGE),
    (["-l", "10", "out.bam", "a.bam", "b.bam"], 1, b"", b"sbx-merge: invalid compression level 10\n"),
    (["-l=x", "out.bam", "a.bam", "b.bam"], 1, b"", b"sbx-merge: invalid compression level x\n"),
    (["--compression-level", "-2", "out.bam", "a.bam", "b.bam"], 1, b"", b"sbx-merge: invalid compression level -2\n"),
    (["--bogus", "out.bam", "a.bam", "b.bam"], 1, b"", b"sbx-merge: Unrecognized option --bogus\n"),
    (["out.bam", "a.bam", "b.bam", "-x"], 1, b"", b"sbx-merge: Unrecognized option -x\n"),
    (["-Hx", "out.bam", "a.bam", "b.bam"], 1, b"", b"sbx-merge: Unrecognized option -Hx\n"),
    (["-n", "out.bam", "a.bam", "b.bam"], 1, b"", b"sbx-merge: Unrecognized option -n\n"),
    (["out.bam", "a.bam", "b.bam", "-l"], 1, b"", b"sbx-merge: Missing value for argument -l.\n"),
    (["out.bam", "a.bam", "b.bam", "--filter"], 1, b"", b"sbx-merge: Missing value for argument --filter.\n"),
    (["out.bam", "a.bam", "b.bam", "-t"], 1, b"", b"sbx-merge: Missing value for argument -t.\n"),
]

# accepted by the options, refused by the open of the first input
REACH_OPEN = [
    ["out.bam", "a.bam", "b.bam"],
    ["-t", "4", "-p", "-v", "out.bam", "a.bam", "b.bam", "c.bam"],
    ["out.bam", "-l", "1", "a.bam", "--nthreads=2", "b.bam", "--show-progress", "--validate-headers"],
    ["--compression-level=0", "-F", "mapping_quality >= 30", "--", "out.bam", "a.bam", "b.bam"],
    ["-H", "out.bam", "a.bam", "b.bam"],
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.merge_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("args,status,stdout,stderr", DECIDED, ids=[" ".join(["sbx-merge"] + c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, status, stdout, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (status, stdout, stderr)
    assert not os.listdir(str(tmp_path))


def test_bad_filter_is_refused_before_any_file_is_opened(tmp_path):
    r = run(["-F", "mapping_quality >=", "out.bam", "a.bam", "b.bam"], tmp_path)
    want = sambamba_amd.SbxError
    with pytest.raises(want) as e:
        sambamba_amd.compile_filter("mapping_quality >=")
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"sbx-merge: " + e.value.msg.encode() + b"\n")
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", REACH_OPEN, ids=[" ".join(["sbx-merge"] + c) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = b"sbx-merge: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == b"sbx-merge: can't open file a.bam\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_output_equal_to_an_input_is_refused(tmp_path):
    path = tmp_path / "b.bam"
    path.write_bytes(b"not even a BAM file")
    (tmp_path / "a.bam").write_bytes(b"nor this")
    for args in (["b.bam", "a.bam", "b.bam"], ["./b.bam", "a.bam", "b.bam", "-l", "3"], [str(path), "a.bam", "b.bam"]):
        r = run(args, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"sbx-merge: the output would overwrite the input b.bam\n")
    assert path.read_bytes() == b"not even a BAM file" and sorted(os.listdir(str(tmp_path))) == ["a.bam", "b.bam"]
