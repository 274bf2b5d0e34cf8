"""What `sambamba sort` needs besides its kernels (sambamba_amd/csrc/sort_core.hpp), compiled for the host with g++ into
tests/native/sort_host.cpp and checked against the Python restatement (tests/sort_ref.py): the 64-bit key K9a packs orders records
exactly as compareCoordinatesAndStrand does, the bits and passes the radix sort is told to look at cover every key, and the
header text of the output is the re-serialisation SamHeader.toSam prints -- no GPU needed."""
import itertools
import os
import struct
import subprocess

import pytest

from tests import sort_ref
from tests.flagstat_ref import inflate
from tests.util import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "native", "sort_host.cpp")
N_REF = 25
GRID = [(ref, pos, strand) for ref in (-1, 0, 1, N_REF - 1) for pos in (-1, 0, 1, 2 ** 28, 2 ** 31 - 1) for strand in (0, 1)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sortc") / "sort_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


def run(exe, args, data=b""):
    return subprocess.run([exe] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def keys_of(exe, triples, n_ref):
    # flags around the strand bit: every other bit set must not matter
    lines = "".join("%d %d %d\n" % (ref, pos, (0x10 if strand else 0) | (0xFEF if k % 2 else 0)) for k, (ref, pos, strand) in enumerate(triples))
    r = run(exe, ["keys", n_ref], lines.encode())
    assert r.returncode == 0, r.stderr
    return [int(x) for x in r.stdout.split()]


def test_key_orders_as_the_comparator(host):
    keys = keys_of(host, GRID, N_REF)
    assert len(keys) == len(GRID)
    for (a, ka), (b, kb) in itertools.product(zip(GRID, keys), repeat=2):
        assert (ka < kb) == sort_ref.before(a, b), (a, b)
        assert (ka == kb) == (not sort_ref.before(a, b) and not sort_ref.before(b, a)), (a, b)


def test_key_is_the_restatements_sort_key(host):
    keys = keys_of(host, GRID, N_REF)
    tuples = [(ref, pos, strand) if ref >= 0 else (N_REF, 0, 0) for ref, pos, strand in GRID]
    assert sorted(range(len(GRID)), key=lambda i: keys[i]) == sorted(range(len(GRID)), key=lambda i: tuples[i])


@pytest.mark.parametrize("n_ref", [1, 2, 25, 3366, 2 ** 20])
def test_key_bits_cover_every_key(host, n_ref):
    grid = [(ref, pos, s) for ref in (-1, 0, min(1, n_ref - 1), n_ref - 1) for pos in (-1, 0, 1, 2 ** 28, 2 ** 31 - 1) for s in (0, 1)]
    keys = keys_of(host, grid, n_ref)
    bits = int(run(host, ["bits", n_ref, 2 ** 31 - 1]).stdout)
    assert bits <= 64 and all(k < (1 << bits) for k in keys)
    assert any(k >= (1 << (bits - 1)) for k in keys)            # and not one bit more than the largest key needs
    # the passes planned for the bits in which these keys differ sort them: every varying bit lies in a digit that is sorted
    k_or, k_and = 0, ~0
    for k in keys:
        k_or |= k
        k_and &= k
    varying = k_or ^ k_and
    out = [int(x) for x in run(host, ["passes", varying]).stdout.split()]
    n_passes, width, shifts = out[0], out[1], out[2:]
    assert n_passes == len(shifts) and shifts == sorted(shifts) and width <= bits
    covered = 0
    for s in shifts:
        covered |= 0xFF << s
    assert varying & ~covered == 0
    assert sorted(keys) == sorted(keys, key=lambda k: [(k >> s) & 0xFF for s in reversed(shifts)])


def test_passes_skip_constant_digits(host):
    assert run(host, ["passes", 0]).stdout.split() == [b"0", b"0"]
    # bits 1 .. 8 and 33 .. 34 vary (positions below 256 on four contigs): two passes, the digits between them are skipped
    varying = 0x1FE | (0x3 << 33)
    out = [int(x) for x in run(host, ["passes", varying]).stdout.split()]
    assert out == [2, 34, 1, 33]


def _bam_text(name):
    stream = inflate(os.path.join(GOLDEN, name + ".bam"))
    l_text = struct.unpack_from("<i", stream, 4)[0]
    return stream[8:8 + l_text].decode()


HAND_MADE = {
    "no_hd": "@SQ\tSN:c1\tLN:1000\n@RG\tID:a\tSM:s\n",
    "hd_go_ss": "@HD\tVN:1.6\tGO:query\tSO:unsorted\tSS:unsorted:md5\n@SQ\tSN:c1\tLN:1000\n",
    "queryname": "@HD\tVN:1.5\tSO:queryname\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:20\n",
    "hd_not_first": "@SQ\tSN:c1\tLN:1000\n@HD\tVN:1.6\tSO:unsorted\n",
    "hd_without_vn": "@HD\tSO:unsorted\n@SQ\tSN:c1\tLN:1000\n",
    "unknown_fields": "@HD\tVN:1.4\tXY:1\n@SQ\tSN:c1\tLN:1000\tXX:foo\tM5:abc\n@RG\tID:a\tzz:1\tSM:s\tPM:m\n@PG\tID:p\tXX:1\tPN:prog\n",
    "duplicated_rg": "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n@RG\tID:a\tSM:first\n@RG\tID:b\tSM:other\n@RG\tID:a\tSM:second\n@PG\tID:p\tVN:1\n@PG\tID:p\tVN:2\n"
                     "@SQ\tSN:c1\tLN:5\n",
    "pi_zero": "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:0\n@RG\tID:a\tPI:0\tSM:s\n@RG\tID:b\tPI:0488\tSM:s\n",
    "co_between": "@HD\tVN:1.6\n@CO\tfirst\tcomment\n@SQ\tSN:c1\tLN:1000\n@CO\t\n@RG\tID:a\n@CO\tlast\n@PG\tID:p\n",
    "sq_out_of_order": "@HD\tVN:1.6\n@SQ\tUR:file:x\tLN:1000\tAH:*\tSN:c1\tSP:human\tM5:0f\tAS:hg\tDS:d\tAN:chr1,one\n"
                       "@RG\tPM:m\tSM:s\tPU:u\tPL:ILLUMINA\tPI:300\tPG:p\tLB:l\tKS:k\tFO:f\tDT:d\tDS:x\tCN:c\tBC:b\tID:a\n@PG\tVN:1\tPP:q\tCL:cmd line\tPN:n\tID:p\n",
    "repeated_field": "@HD\tVN:1.0\tVN:1.6\n@SQ\tSN:a\tSN:b\tLN:5\n",
    "short_lines_and_no_newline": "@HD\tVN:1.6\n\n@\n@SQ\tSN:c1\tLN:1000",
    "zero_padded": "@HD\tVN:1.6\n@SQ\tSN:c1\tLN:1000\n\0\0\0",
    "empty": "",
}


@pytest.mark.parametrize("name", ["issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates"])
def test_header_text_of_the_fixtures(host, name):
    text = _bam_text(name)
    r = run(host, ["header"], text.encode())
    assert r.returncode == 0, r.stderr
    want = sort_ref.header_text(text)
    assert r.stdout.decode() == want
    assert want.startswith("@HD\tVN:") and want.split("\n")[0].endswith("\tSO:coordinate")
    assert want.count("@SQ\t") == text.count("@SQ\t")


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_header_text_hand_made(host, name):
    text = HAND_MADE[name]
    r = run(host, ["header"], text.encode())
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == sort_ref.header_text(text)


def test_header_text_known_answers(host):
    """The restatement itself, pinned on cases worked out by hand from header.d."""
    assert sort_ref.header_text("") == "@HD\tVN:1.3\tSO:coordinate\n"
    assert sort_ref.header_text(HAND_MADE["hd_go_ss"]) == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:1000\n"
    assert sort_ref.header_text(HAND_MADE["hd_not_first"]) == "@HD\tVN:1.3\tSO:coordinate\n@SQ\tSN:c1\tLN:1000\n"
    assert sort_ref.header_text(HAND_MADE["duplicated_rg"]) == ("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:1000\n@RG\tID:a\tSM:first\n"
                                                                "@RG\tID:b\tSM:other\n@PG\tID:p\tVN:1\n")
    assert sort_ref.header_text(HAND_MADE["pi_zero"]) == "@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\n@RG\tID:a\tSM:s\n@RG\tID:b\tPI:488\tSM:s\n"
    assert sort_ref.header_text(HAND_MADE["co_between"]) == ("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:c1\tLN:1000\n@RG\tID:a\n@PG\tID:p\n"
                                                             "@CO\tfirst\tcomment\n@CO\t\n@CO\tlast\n")
    assert sort_ref.header_text(HAND_MADE["sq_out_of_order"]).split("\n")[1] == \
        "@SQ\tSN:c1\tLN:1000\tAN:chr1,one\tAS:hg\tDS:d\tM5:0f\tSP:human\tUR:file:x\tAH:*"


def test_header_text_refusals(host):
    assert run(host, ["header"], b"@HD\tVN:1.6\nnot a header line\n").returncode == 3
    assert run(host, ["header"], b"@HD\tVN:1.6\n@SQ\tSN:c1\tLN:12x\n").returncode == 3


def test_header_text_through_the_library():
    import sambamba_amd
    for text in HAND_MADE.values():
        assert sambamba_amd.sort_header_text(text) == sort_ref.header_text(text)
    with pytest.raises(sambamba_amd.SbxError):
        sambamba_amd.sort_header_text("junk line\n")
