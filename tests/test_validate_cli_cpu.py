"""`sbx-validate` and the report text without a GPU: the usage and the exit statuses the command line alone decides,
sbx_format_validate_report byte for byte, and the -v option where it is taken (sbx-sam) and where it stays refused (sbx-view)."""
import subprocess

import pytest

import sambamba_amd

USAGE_HEAD = b"Usage: sbx-validate [options] <input.bam> [<input2.bam> [...]]\n"


def run(exe, args, cwd):
    r = subprocess.run([exe] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return r.returncode, r.stdout, r.stderr


@pytest.mark.parametrize("args", [[], ["-t", "4"], ["-p"], ["--nthreads=2", "--show-progress"], ["--"]])
def test_without_a_file_the_usage_and_status_1(tmp_path, args):
    status, out, err = run(sambamba_amd.validate_cli_path(), args, tmp_path)
    assert status == 1 and out == b""
    assert err.startswith(USAGE_HEAD) and b"-t, --nthreads=N" in err and b"-p, --show-progress" in err


@pytest.mark.parametrize("args, stderr", [
    (["-x", "in.bam"], b"sbx-validate: Unrecognized option -x\n"),
    (["in.bam", "--bogus"], b"sbx-validate: Unrecognized option --bogus\n"),
    (["-px", "in.bam"], b"sbx-validate: Unrecognized option -px\n"),
    (["in.bam", "-t"], b"sbx-validate: Missing value for argument -t.\n"),
])
def test_refused_command_lines(tmp_path, args, stderr):
    assert run(sambamba_amd.validate_cli_path(), args, tmp_path) == (1, b"", stderr)


def test_a_file_that_is_not_there(tmp_path):
    status, out, err = run(sambamba_amd.validate_cli_path(), ["-t", "2", "missing.bam", "-p"], tmp_path)
    assert status == 1 and out == b"" and err.startswith(b"sbx-validate: ") and err.endswith(b"\n")


def test_report_text_byte_for_byte():
    counts = {"name-chars": 2, "position": 1, "tag-duplicate": 7, "malformed": 3}
    first = {"ordinal": 41, "mask": 1 << 1 | 1 << 7 | 1 << 9, "name": b"a\tb\x80\\c~!@ "}
    text = sambamba_amd.format_validate_report("dir/some file.bam", 1000, 9, counts, first)
    assert text == (b"file\tdir/some file.bam\nrecords\t1000\ninvalid\t9\n"
                    b"name-empty\t0\nname-chars\t2\nposition\t1\nqualities\t0\ncigar-hard\t0\ncigar-soft\t0\ncigar-length\t0\n"
                    b"tag-value\t0\ntag-duplicate\t7\nmalformed\t3\n"
                    b"first-invalid\t41\ta\\x09b\\x80\\x5Cc~!@\\x20\tname-chars,tag-value,malformed\n")
    clean = sambamba_amd.format_validate_report("x.bam", 5, 0, {})
    assert clean == (b"file\tx.bam\nrecords\t5\ninvalid\t0\nname-empty\t0\nname-chars\t0\nposition\t0\nqualities\t0\ncigar-hard\t0\n"
                     b"cigar-soft\t0\ncigar-length\t0\ntag-value\t0\ntag-duplicate\t0\nmalformed\t0\n")
    # a first record without a name (malformed), and the longest name
    assert sambamba_amd.format_validate_report("x", 1, 1, {"malformed": 1}, {"ordinal": 0, "mask": 512, "name": b""}).endswith(
        b"first-invalid\t0\t\tmalformed\n")
    long_name = sambamba_amd.format_validate_report("x", 1, 1, {"position": 1}, {"ordinal": 0, "mask": 4, "name": b"n" * 254})
    assert long_name.endswith(b"first-invalid\t0\t" + b"n" * 254 + b"\tposition\n")
    assert tuple(sambamba_amd.VALIDATE_CLASSES) == ("name-empty", "name-chars", "position", "qualities", "cigar-hard", "cigar-soft",
                                                    "cigar-length", "tag-value", "tag-duplicate", "malformed")


def test_sbx_view_still_refuses_valid(tmp_path):
    for args in (["-v", "-f", "bam", "in.bam"], ["-c", "in.bam", "--valid"]):
        assert run(sambamba_amd.view_cli_path(), args, tmp_path) == (1, b"", b"sbx-view: option -v / --valid is not supported\n")


def test_sbx_sam_takes_valid(tmp_path):
    # the option is parsed and the call reaches the open of a file that is not there; with text attached it is no option
    for args in (["-v", "-c", "missing.bam"], ["missing.bam", "--valid"], ["-v", "-f", "bam", "missing.bam", "-o", "out.bam"]):
        status, out, err = run(sambamba_amd.sam_cli_path(), args, tmp_path)
        assert status == 1 and out == b"" and err.startswith(b"sbx-sam: ") and b"not supported" not in err and b"Unrecognized" not in err
    assert run(sambamba_amd.sam_cli_path(), ["-vx", "-c", "missing.bam"], tmp_path) == (1, b"", b"sbx-sam: Unrecognized option -vx\n")
    status, out, err = run(sambamba_amd.sam_cli_path(), [], tmp_path)
    assert status == 0 and b"-v, --valid\n                    output only valid alignments\n" in err
    assert b"-S, --sam-input\n                    not supported\n" in err


def test_abi_knows_the_new_structs():
    import ctypes as C
    from sambamba_amd._lib import ValidateReport, ValidateStats, ViewRequest
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_view_request") == C.sizeof(ViewRequest) == 96
    assert L.sbx_abi_sizeof(b"sbx_validate_report") == C.sizeof(ValidateReport) == 368
    assert L.sbx_abi_sizeof(b"sbx_validate_stats") == C.sizeof(ValidateStats) == 48
    assert ViewRequest.struct_size.offset == 0 and ViewRequest.valid_only.offset == 88
