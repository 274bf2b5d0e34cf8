"""The option policy of sbx-view, pinned byte for byte in the manner of tests/test_markdup_cli_cpu.py: it scans its arguments with
csrc/cli_opts.hpp, refuses the output formats it does not have (sam -- the reference's default --, json, unpack, msgpack, cram), -v and
-S by name, refuses -L together with a region, a bad --num-filter, -s, --subsampling-seed and -l, accepts and ignores -t, -p, -T and
-h, and prints the usage with exit status 0 when it has no file name (as view_main does).  Every vector is decided before a device is
used, or ends in the library's open."""
import os
import subprocess

import pytest

import sambamba_amd

USAGE = (
    b"Usage: sbx-view [options] <input.bam> [region1 [...]]\n"
    b"\n"
    b"Selects records of a BAM file, as `sambamba view` does, on the GPU; writes a BAM (-f bam) or their number (-c).\n"
    b"\n"
    b"Options: -F, --filter=FILTER\n"
    b"                    set custom filter for alignments\n"
    b"         --num-filter=NUMFILTER\n"
    b"                    filter flag bits; 'i1/i2' corresponds to -f i1 -F i2 samtools arguments;\n"
    b"                    either of the numbers can be omitted\n"
    b"         -f, --format=bam\n"
    b"                    output format; only bam is supported (sam, the reference's default, json, unpack,\n"
    b"                    msgpack and cram are not): give -f bam or -c\n"
    b"         -h, --with-header\n"
    b"                    accepted; the header is always written for BAM output\n"
    b"         -H, --header\n"
    b"                    output only header to stdout, as SAM\n"
    b"         -I, --reference-info\n"
    b"                    output to stdout only reference names and lengths in JSON\n"
    b"         -L, --regions=FILENAME\n"
    b"                    output only reads overlapping one of regions from the BED file\n"
    b"         -c, --count\n"
    b"                    output to stdout only count of matching records, hHI are ignored\n"
    b"         -l, --compression-level\n"
    b"                    specify compression level (from 0 to 9)\n"
    b"         -o, --output-filename\n"
    b"                    specify output filename (default, and '-': stdout)\n"
    b"         -s, --subsample=FRACTION\n"
    b"                    subsample reads (read pairs)\n"
    b"         --subsampling-seed=SEED\n"
    b"                    set seed for subsampling\n"
    b"         -t, --nthreads=NTHREADS, -p, --show-progress, -T, --ref-filename=FASTA\n"
    b"                    accepted for compatibility\n"
    b"         -v, --valid, -S, --sam-input\n"
    b"                    not supported\n"
    b"\n"
    b"Regions are 'chr', 'chr:beg-end' or '*' (reads without a reference); at most 1024 may be listed, a BED file has no limit.\n"
    b"A read that overlaps several listed regions is written once per region.  No index is needed; the whole file is read.\n")


def unsupported(fmt):
    return b"sbx-view: output format " + fmt + b" is not supported yet: use -f bam or -c\n"


NUM_FILTER = b": expected i1/i2, two numbers from 0 to 65535, either of which may be missing\n"

# (arguments, exit status, stdout, stderr): decided by the command line alone
DECIDED = [
    ([], 0, b"", USAGE),
    (["-c"], 0, b"", USAGE),
    (["-f", "bam", "-t", "4"], 0, b"", USAGE),
    (["--"], 0, b"", USAGE),
    (["in.bam"], 1, b"", unsupported(b"sam")),
    (["-h", "in.bam", "chr1"], 1, b"", unsupported(b"sam")),
    (["-f", "sam", "in.bam"], 1, b"", unsupported(b"sam")),
    (["--format=json", "in.bam"], 1, b"", unsupported(b"json")),
    (["in.bam", "-f", "unpack"], 1, b"", unsupported(b"unpack")),
    (["-fmsgpack", "in.bam"], 1, b"", unsupported(b"msgpack")),
    (["-f=cram", "in.bam"], 1, b"", unsupported(b"cram")),
    (["-f", "xml", "in.bam"], 1, b"", b"sbx-view: output format must be one of sam, bam, json\n"),
    (["-v", "-f", "bam", "in.bam"], 1, b"", b"sbx-view: option -v / --valid is not supported\n"),
    (["-c", "in.bam", "--valid"], 1, b"", b"sbx-view: option -v / --valid is not supported\n"),
    (["-S", "in.sam"], 1, b"", b"sbx-view: option -S / --sam-input is not supported\n"),
    (["--sam-input", "-c", "in.sam"], 1, b"", b"sbx-view: option -S / --sam-input is not supported\n"),
    (["-c", "-L", "r.bed", "in.bam", "chr1"], 1, b"", b"sbx-view: specifying both region and BED filename is disallowed\n"),
    (["-f", "bam", "--regions=r.bed", "in.bam", "chr1:1-10", "*"], 1, b"", b"sbx-view: specifying both region and BED filename is disallowed\n"),
    (["-c", "--num-filter=65536", "in.bam"], 1, b"", b"sbx-view: invalid --num-filter 65536" + NUM_FILTER),
    (["-c", "--num-filter", "-1", "in.bam"], 1, b"", b"sbx-view: invalid --num-filter -1" + NUM_FILTER),
    (["-c", "--num-filter=a/b", "in.bam"], 1, b"", b"sbx-view: invalid --num-filter a/b" + NUM_FILTER),
    (["-c", "-s", "-0.1", "in.bam"], 1, b"", b"sbx-view: invalid subsampling fraction -0.1\n"),
    (["-c", "-s", "nan", "in.bam"], 1, b"", b"sbx-view: invalid subsampling fraction nan\n"),
    (["-c", "--subsample=half", "in.bam"], 1, b"", b"sbx-view: invalid subsampling fraction half\n"),
    (["-c", "-s", "0.5", "--subsampling-seed=-3", "in.bam"], 1, b"", b"sbx-view: invalid subsampling seed -3\n"),
    (["-c", "-s", "0.5", "--subsampling-seed", "12x", "in.bam"], 1, b"", b"sbx-view: invalid subsampling seed 12x\n"),
    (["-f", "bam", "-l", "10", "in.bam"], 1, b"", b"sbx-view: invalid compression level 10\n"),
    (["-f", "bam", "-l=x", "in.bam"], 1, b"", b"sbx-view: invalid compression level x\n"),
    (["-f", "bam", "in.bam", "-l"], 1, b"", b"sbx-view: Missing value for argument -l.\n"),
    (["-c", "in.bam", "--num-filter"], 1, b"", b"sbx-view: Missing value for argument --num-filter.\n"),
    (["--bogus", "in.bam"], 1, b"", b"sbx-view: Unrecognized option --bogus\n"),
    (["--throw-error", "in.bam"], 1, b"", b"sbx-view: Unrecognized option --throw-error\n"),
    (["-cx", "in.bam"], 1, b"", b"sbx-view: Unrecognized option -cx\n"),
    (["-c", "-F", "mapping_quality >=", "in.bam"], 1, b"", None),
    (["-c", "in.bam"] + ["chr1:%d-%d" % (k + 1, k + 10) for k in range(1025)], 1, b"",
     b"sbx-view: too many regions (1025): at most 1024 may be listed; use -L with a BED file\n"),
]

# accepted by the options, refused by the open of the input
REACH_OPEN = [
    ["-c", "in.bam"],
    ["-f", "bam", "in.bam"],
    ["-f", "bam", "-o", "out.bam", "in.bam"],
    ["-c", "-t", "4", "-p", "-T", "ref.fa", "-h", "in.bam"],
    ["in.bam", "--format=bam", "--nthreads=2", "--show-progress", "--ref-filename=ref.fa", "--with-header", "-l", "1", "--output-filename=out.bam"],
    ["-c", "-f", "json", "in.bam"],                                                   # -c ignores the format
    ["-c", "--num-filter=4/", "-F", "not duplicate", "-s", "0.25", "--subsampling-seed=18446744073709551615", "in.bam", "chr1:1-10", "*"],
    ["-c", "--num-filter=", "-s", "1.5", "in.bam"],
    ["-c", "-L", "r.bed", "in.bam"],
    ["-H", "in.bam"],
    ["-I", "in.bam"],
    ["-c", "--", "in.bam"],
    ["-c", "in.bam"] + ["chr1:%d-%d" % (k + 1, k + 10) for k in range(1024)],
]


def run(args, cwd):
    return subprocess.run([sambamba_amd.view_cli_path()] + args, cwd=str(cwd), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                          stderr=subprocess.PIPE, timeout=120)


def _id(args):
    s = " ".join(["sbx-view"] + args)
    return s if len(s) < 80 else s[:60] + "...(%d arguments)" % len(args)


@pytest.mark.parametrize("args,status,stdout,stderr", DECIDED, ids=[_id(c[0]) for c in DECIDED])
def test_outcome_decided_by_the_command_line(tmp_path, args, status, stdout, stderr):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (status, stdout)
    if stderr is None:
        assert r.stderr.startswith(b"sbx-view: ") and r.stderr.count(b"\n") == 1
    else:
        assert r.stderr == stderr
    assert not os.listdir(str(tmp_path))


@pytest.mark.parametrize("args", REACH_OPEN, ids=[_id(c) for c in REACH_OPEN])
def test_accepted_command_line_reaches_the_open(tmp_path, args):
    r = run(args, tmp_path)
    assert (r.returncode, r.stdout) == (1, b"")
    no_device = b"sbx-view: no HIP device available (libsbx_depth has no CPU fallback): "
    assert r.stderr == b"sbx-view: can't open file in.bam\n" or (r.stderr.startswith(no_device) and r.stderr.count(b"\n") == 1)
    assert not os.listdir(str(tmp_path))            # nothing was created on the way


def test_output_equal_to_input_is_refused(tmp_path):
    path = tmp_path / "in.bam"
    path.write_bytes(b"not even a BAM file")
    for args in (["-f", "bam", "-o", "in.bam", "in.bam"], ["-f", "bam", "in.bam", "-o", "./in.bam"], ["-f", "bam", "-o", str(path), "in.bam"]):
        r = run(args, tmp_path)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", b"sbx-view: the output would overwrite the input in.bam\n")
    assert path.read_bytes() == b"not even a BAM file" and os.listdir(str(tmp_path)) == ["in.bam"]


def test_num_filter_through_the_library():
    assert sambamba_amd.view_num_filter("4/") == (4, 0)
    assert sambamba_amd.view_num_filter("/4") == (0, 4)
    assert sambamba_amd.view_num_filter("3/1024") == (3, 1024)
    assert sambamba_amd.view_num_filter("") == (0, 0)
    for text in ("65536", "-1", "a/b"):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.view_num_filter(text)
        assert ei.value.code == -1
