"""The option policy of sbx-subsample, pinned byte for byte in the manner of tests/test_fixbins_cli_cpu.py: without arguments the
usage goes to stdout with exit status 1 (as subsample_main does), the reference's refusals come in its order and words, more than one
input and an output that is the input are refused by name.  Every vector is decided before a device is used, or ends in the
library's open; nothing is created on the way."""
import os
import subprocess

import pytest

import sambamba_amd

OK = ["--type", "fasthash", "--max-cov", "10", "-o", "out.bam"]

# (arguments, exit status, stderr): decided by the command line alone, nothing on stdout
DECIDED = [
    (["in.bam"], b"sbx-subsample: Output not defined\n"),
    (["--type", "fasthash", "--max-cov", "10", "in.bam"], b"sbx-subsample: Output not defined\n"),
    (["-o", "out.bam", "in.bam"], b"sbx-subsample: Algorithm not defined\n"),
    (["-o", "out.bam", "--type", "hash1", "--max-cov", "10", "in.bam"], b"sbx-subsample: Algorithm not defined\n"),
    (["-o", "out.bam", "--type=fasthash", "in.bam"], b"sbx-subsample: Maximum coverage not set\n"),
    (["-oout.bam", "--type=fasthash", "--max-cov=0", "in.bam"], b"sbx-subsample: Maximum coverage not set\n"),
    (["--output=out.bam", "--type=fasthash", "--max-cov", "-3", "in.bam"], b"sbx-subsample: Maximum coverage not set\n"),
    (["-o", "out.bam", "--type=fasthash", "--max-cov", "ten", "in.bam"], b"sbx-subsample: invalid maximum coverage ten\n"),
    (["-o", "out.bam", "--type=fasthash", "--max-cov", "4294967296", "in.bam"], b"sbx-subsample: invalid maximum coverage 4294967296\n"),
    (OK + ["-l", "10", "in.bam"], b"sbx-subsample: invalid compression level 10\n"),
    (OK + ["-l=x", "in.bam"], b"sbx-subsample: invalid compression level x\n"),
    (OK, b"sbx-subsample: no input file\n"),
    (OK + ["a.bam", "b.bam"], b"sbx-subsample: more than one input file is not supported: out.bam would be overwritten once per input (a.bam, b.bam)\n"),
    (OK + ["a.bam", "b.bam", "c.bam"],
     b"sbx-subsample: more than one input file is not supported: out.bam would be overwritten once per input (a.bam, b.bam, ...)\n"),
    (OK + ["out.bam"], b"sbx-subsample: Input file can not be same as output file out.bam\n"),
    (OK + ["--bogus", "in.bam"], b"sbx-subsample: Unrecognized option --bogus\n"),
    (OK + ["-x", "in.bam"], b"sbx-subsample: Unrecognized option -x\n"),
    (OK + ["-rx", "in.bam"], b"sbx-subsample: Unrecognized option -rx\n"),
    (["in.bam", "--type", "fasthash", "--max-cov", "10", "-o"], b"sbx-subsample: Missing value for argument -o.\n"),
    (["in.bam", "-o", "out.bam", "--type", "fasthash", "--max-cov"], b"sbx-subsample: Missing value for argument --max-cov.\n"),
]

# accepted by the options, refused by the open of the input
REACH_OPEN = [
    OK + ["in.bam"],
    ["in.bam"] + OK + ["-r"],
    ["--type=fasthash", "--max-cov=2147483647", "-oout.bam", "--remove", "-l", "1", "--logging", "debug", "in.bam"],
    OK + ["-l9", "--", "in.bam"],
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.subsample_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


def test_no_arguments_prints_the_usage_on_stdout_with_status_1(tmp_path):
    r = run([], tmp_path)
    assert r.returncode == 1 and r.stderr == b""
    text = r.stdout.decode()
    assert text.startswith("\nUsage: sbx-subsample [options] <input.bam>\n")
    for word in ("--type [fasthash]", "--max-cov [depth]", "-o, --output fn", "-r, --remove", "-l level", "--logging type"):
        assert word in text
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args,stderr", DECIDED, ids=[" ".join(["sbx-subsample"] + c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", stderr)
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", REACH_OPEN, ids=[" ".join(["sbx-subsample"] + c) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = b"sbx-subsample: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == b"sbx-subsample: can't open file in.bam\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_output_equal_to_input_by_another_name(tmp_path):
    path = tmp_path / "in.bam"
    path.write_bytes(b"not even a BAM file")
    for out in ("in.bam", "./in.bam", str(path)):
        r = run(["--type", "fasthash", "--max-cov", "5", "-o", out, "in.bam"], tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"sbx-subsample: Input file can not be same as output file in.bam\n")
    assert path.read_bytes() == b"not even a BAM file" and os.listdir(str(tmp_path)) == ["in.bam"]


def test_binding_names_the_binary_and_the_abi():
    import ctypes as C
    from sambamba_amd._lib import EXPORTS, SubsampleStats
    assert os.path.basename(sambamba_amd.subsample_cli_path()) == "sbx-subsample" and os.access(sambamba_amd.subsample_cli_path(), os.X_OK)
    L = sambamba_amd.lib()
    assert "sbx_subsample" in EXPORTS and hasattr(L, "sbx_subsample")
    assert L.sbx_abi_sizeof(b"sbx_subsample_stats") == C.sizeof(SubsampleStats) == 10 * 8 + 2 * 4 + 7 * 8
    # the arguments are checked before a device is asked for
    for kw, word in (({"max_cov": 0}, "Maximum coverage not set"), ({"max_cov": 5, "level": 12}, "compression level")):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.subsample("in.bam", "out.bam", **kw)
        assert ei.value.code == -1 and word in ei.value.msg
