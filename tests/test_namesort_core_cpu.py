"""The read-name orders of `sambamba sort -n / -N / -M` (sambamba_amd/csrc/namesort_core.hpp), compiled for the host with g++ into
tests/native/namesort_host.cpp: the comparators against the reference's known answers, the key encoder against the comparators over
every short string and over seeded long names, the two sinks of the encoder, the HI lookup -- and once more under AddressSanitizer
and UBSan.  The Python restatement the device tests compare against (tests/namesort_ref.py) is held to the same known answers.
Then the options of `sbx-nsort`, which are decided before any device call.  No GPU needed."""
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import namesort_ref as ref
from tests.util import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "native", "namesort_host.cpp")
HEADER = os.path.join(ROOT, "sambamba_amd", "csrc", "namesort_core.hpp")

KNOWN = [("BC0123", "BC01234", -1), ("BC0123", "BC0123Z", -1), ("BC01234", "BC01234", 0), ("BC0123DEF45", "BC01234DEF45", -1),
         ("BC01236DEF45", "BC01234DEF45", 1), ("BC012", "BC0012", -1), ("BC0012DE0034", "BC0012DE34", 1), ("BC12DE0034", "BC012DE34", -1),
         ("1235", "1234", 1)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nsc") / "namesort_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nsc_san") / "namesort_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, *args, data=None):
    r = subprocess.run([exe] + list(args), input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout.decode()[-3000:], r.stderr.decode()[-3000:])
    return r.stdout.decode()


def checked(out):
    words = out.split()
    assert words[-4] == "checked" and words[-2:] == ["bad", "0"], out[-2000:]
    return int(words[-3])


def test_known_answers(host):
    assert checked(run(host, "known")) == 9 + 8 + 32


def test_restatement_known_answers():
    sign = lambda v: (v > 0) - (v < 0)
    for a, b, want in KNOWN:
        assert sign(ref.mixed_str_compare(a.encode(), b.encode())) == want, (a, b)
        assert sign(ref.mixed_str_compare(b.encode(), a.encode())) == -want, (a, b)


def test_every_short_string(host):
    # 2801 strings, both orders: their keys through both sinks, then every ordered pair
    assert checked(run(host, "exhaustive")) == 2 * (2801 + 2801 * 2801)


def test_seeded_long_names(host):
    n = checked(run(host, "random", "20240917", "3000"))
    assert n >= 2 * (3000 + 3000 * 3000)


def test_under_sanitizers(host_san):
    checked(run(host_san, "known"))
    assert checked(run(host_san, "exhaustive")) == 2 * (2801 + 2801 * 2801)
    assert checked(run(host_san, "random", "7", "700")) >= 2 * (700 + 700 * 700)
    hi_lookup(host_san)


def hi_cases():
    """(aux bytes, ok, value)"""
    t = bamgen.tag_num
    other = bamgen.tag_z("RG", "g1") + t("NH", "C", 4) + bamgen.tag_bytes("XB", [1, 2, 3]) + t("XA", "A", "q") + t("XF", "f", 1.5)
    cases = [(b"", 1, 0), (other, 1, 0)]
    for ty, lo, hi in (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", -2**31, 2**31 - 1), ("I", 0, 2**31 - 1)):
        for v in (lo, hi, 1):
            cases.append((other + t("HI", ty, v), 1, v))
            cases.append((t("HI", ty, v) + other, 1, v))
    cases.append((t("HI", "I", 2**31), 0, None))                      # does not fit int
    cases.append((t("HI", "I", 2**32 - 1), 0, None))
    cases.append((t("HI", "C", 3) + t("HI", "C", 9), 1, 3))          # the first one counts
    cases.append((t("HI", "C", 3) + b"XX", 1, 3))                    # (nothing behind HI is looked at)
    for bad in (bamgen.tag_z("HI", "7"), t("HI", "f", 1.0), t("HI", "A", "1"), bamgen.tag_bytes("HI", [1]), b"HIH00\0"):
        cases.append((other + bad, 0, None))
    # tags that run past the record: cut inside the key, the type, the value, a string without NUL, an array longer than the rest
    whole = other + t("HI", "i", 70000)
    for cut in (1, 2, 4, len(other) - 1, len(other) + 1, len(other) + 2, len(other) + 3, len(other) + 6):
        cases.append((whole[:cut], 0, None))
    cases.append((b"RGZg1", 0, None))
    cases.append((b"XBBC" + struct.pack("<I", 100) + b"\1\2", 0, None))
    cases.append((b"XBBC" + struct.pack("<I", 0xFFFFFFFF), 0, None))
    cases.append((b"XQ?\0" + t("HI", "C", 1), 0, None))               # a type nobody knows
    return cases


def hi_lookup(exe):
    cases = hi_cases()
    out = run(exe, "hi", data="".join((aux.hex() or "-") + "\n" for aux, _, _ in cases).encode())
    rows = [tuple(int(x) for x in line.split()) for line in out.splitlines()]
    assert len(rows) == len(cases)
    for (aux, ok, value), (got_ok, got_value) in zip(cases, rows):
        assert got_ok == ok, aux
        if ok:
            assert got_value == value, aux
        # the restatement agrees
        rec = bamgen.make_record(0, 1, "4M", "ACGT", 30, name="r", tags=aux)
        if ok:
            assert ref.hi_of(rec) == value, aux
        else:
            with pytest.raises(ValueError):
                ref.hi_of(rec)


def test_hi_lookup(host):
    hi_lookup(host)


def test_restatement_orders_match_mates_fixture():
    # sort -n -M / -N -M of the reference's own fixture: names ascending, then HI, then flag (first mate before second)
    from tests.flagstat_ref import inflate
    from tests import sort_ref
    stream = inflate(os.path.join(GOLDEN, "match_mates.bam"))
    for order in (ref.LEX, ref.NATURAL):
        out = ref.expected_stream(stream, order, True)
        text, _, _, recs = sort_ref.split_stream(out)
        assert text.startswith(b"@HD\tVN:1.3\tSO:queryname\n@SQ\t")
        keys = [(ref.name_of(r), ref.hi_of(r), ref.flag_of(r)) for r in recs]
        assert len(keys) == 22 and keys == sorted(keys)
        assert sorted(recs) == sorted(sort_ref.split_stream(stream)[3])


# ---- sbx-nsort: decided before any device call ----
NSORT_USAGE = (
    b"Usage: sbx-nsort [options] <input.bam>\n\n"
    b"Sorts a BAM file by coordinate or by read name, as `sambamba sort` does, on the GPU.\n\n"
    b"Options: -o, --out=OUTPUTFILE\n"
    b"               output file name; if not provided, the result is written to a file with .sorted.bam extension\n"
    b"         -l, --compression-level=COMPRESSION_LEVEL\n"
    b"               level of compression for sorted BAM, from 0 to 9\n"
    b"         -F, --filter=FILTER\n"
    b"               keep only reads that satisfy FILTER\n"
    b"         -m, --memory-limit=LIMIT, --tmpdir=TMPDIR, -u, --uncompressed-chunks, -t, --nthreads=NTHREADS, -p, --show-progress\n"
    b"               accepted for compatibility; the file is sorted in GPU memory\n"
    b"         -n, --sort-by-name\n"
    b"               sort by read name instead of coordinate (lexicographical order)\n"
    b"         -N, --natural-sort\n"
    b"               sort by read name instead of coordinate (so-called 'natural' sort as in samtools)\n"
    b"         -M, --match-mates\n"
    b"               pull mates of the same alignment together when sorting by read name\n"
    b"         --sort-picard\n"
    b"               not supported\n")


def nsort(args):
    import sambamba_amd
    return subprocess.run([sambamba_amd.nsort_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_nsort_option_handling(tmp_path):
    path = os.path.join(GOLDEN, "match_mates.bam")
    out = str(tmp_path / "o.bam")
    both = b"sbx-nsort: only one of -n and -N and -s parameters can be provided\n"
    alone = b"sbx-nsort: -M option only works in combination with either -n or -N\n"
    cases = [(["-n", "-N"], both), (["--sort-by-name", "--natural-sort", "-M"], both), (["-N", "-o", out, path, "-n"], both),
             (["-M"], alone), (["--match-mates", "-o", out, path], alone),
             (["--sort-picard", "-o", out, path], b"sbx-nsort: option --sort-picard is not supported\n"),
             (["-n", "--sort-picard", path], b"sbx-nsort: option --sort-picard is not supported\n"),
             (["-nM", path], b"sbx-nsort: Unrecognized option -nM\n"),
             (["-n", "-l", "12", "-o", out, path], b"sbx-nsort: invalid compression level 12\n"),
             (["-N", "-o"], b"sbx-nsort: Missing value for argument -o.\n"),
             ([], NSORT_USAGE), (["-n", "-M"], NSORT_USAGE)]
    for args, stderr in cases:
        r = nsort(args)
        assert (r.returncode, r.stdout, r.stderr) == (1, b"", stderr), args
        assert not os.path.exists(out)


def test_python_arguments():
    import sambamba_amd
    with pytest.raises(ValueError):
        sambamba_amd.sort_bam("a.bam", "b.bam", order="queryname", index=True)
    with pytest.raises(ValueError):
        sambamba_amd.sort_bam("a.bam", "b.bam", order="picard")
    with pytest.raises(ValueError):
        sambamba_amd.sort_bam("a.bam", "b.bam", match_mates=True)
    assert "sbx_sort_bam_by_name" in sambamba_amd._lib.EXPORTS and os.path.exists(sambamba_amd.nsort_cli_path())
    assert os.path.exists(HEADER)
