"""What `sambamba sort` needs besides its kernels (sambamba_amd/csrc/sort_core.hpp), compiled for the host with g++ into
tests/native/sort_host.cpp and checked against the Python restatement (tests/sort_ref.py): the 64-bit key K9a packs orders records
exactly as compareCoordinatesAndStrand does, the bits and passes the radix sort is told to look at cover every key, and the
header text of the output is the re-serialisation SamHeader.toSam prints, and the piece arithmetic of the output tail (the bounds of
k_piece_bounds, the record range of a piece, the clip of K9c) puts every byte of the stream into exactly one place of exactly one
piece -- no GPU needed."""
import bisect
import itertools
import os
import random
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


# ---- the pieces of the output stream ------------------------------------------------------------------------------------------------
PIECE_BLOCK = 64               # a "BGZF payload" small enough to enumerate: the cap is a parameter of the functions under test


def _piece_cases(cap):
    """name -> (header length, record lengths); the boundaries are at the multiples of cap."""
    rng = random.Random(cap)
    cases = {}
    for seed in range(4):
        cases["random%d" % seed] = (rng.randrange(0, 3 * cap), [rng.randrange(36, 201) for _ in range(rng.randrange(1, 80))])
    # every record 64 bytes behind a header of a multiple of 64: every boundary is a record's edge; one byte more: none is
    cases["boundary_on_record_edges"] = (cap, [PIECE_BLOCK] * 13)
    cases["boundary_one_byte_into_records"] = (cap + 1, [PIECE_BLOCK] * 13)
    cases["boundary_one_byte_before_the_edge"] = (cap - 1, [PIECE_BLOCK] * 13)
    cases["record_longer_than_two_pieces"] = (17, [40, 2 * cap + 100, 50, 3 * cap, 36])
    cases["record_is_exactly_a_piece"] = (cap, [cap, 2 * cap, 36])
    cases["header_longer_than_a_piece"] = (cap + 37, [40, 50, 60])
    cases["header_of_two_whole_pieces"] = (2 * cap, [40, 50, 60])
    cases["no_records"] = (2 * cap + 5, [])
    cases["no_records_header_is_one_piece"] = (cap, [])
    cases["nothing_at_all"] = (0, [])
    lens = [rng.randrange(36, 201) for _ in range(20)]
    hlen = 29
    lens.append(5 * cap - (hlen + sum(lens)) % cap if (hlen + sum(lens)) % cap else 4 * cap)
    assert (hlen + sum(lens)) % cap == 0
    cases["total_is_a_multiple_of_the_cap"] = (hlen, lens)
    return cases


@pytest.mark.parametrize("blocks", [1, 2, 3])
def test_pieces_hold_every_byte_of_the_stream_once(host, blocks):
    cap = blocks * PIECE_BLOCK
    for name, (hlen, lens) in _piece_cases(cap).items():
        r = run(host, ["pieces", hlen, cap], " ".join(map(str, lens)).encode())
        assert r.returncode == 0, (name, r.stderr)
        want = bytes(0x80 | (j % 127) for j in range(hlen)) + b"".join(bytes((i * 131 + j * 7 + 3) % 127 for j in range(l)) for i, l in enumerate(lens))
        total, n = len(want), len(lens)
        # the concatenation of the pieces is header + records
        assert r.stdout == want, name
        lines = r.stderr.decode().splitlines()
        pieces = [[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("piece ")]
        assert len(pieces) == (total + cap - 1) // cap, name
        for k, (kk, p0, p1, r0, r1, unwritten, twice, outside) in enumerate(pieces):
            assert (kk, p0, p1) == (k, k * cap, min(total, (k + 1) * cap)), name
            # every byte of the piece written exactly once, none outside [0, p1 - p0)
            assert (unwritten, twice, outside) == (0, 0, 0), (name, k)
            assert 0 <= r0 <= r1 <= n, (name, k)
        # the bounds are what their definition says: the first record that ends behind byte k * cap, n when none does
        ends = list(itertools.accumulate(lens, initial=hlen))[1:]
        bounds = [int(x) for x in lines[0].split()[1:]]
        assert lines[0].startswith("bounds") and bounds == [bisect.bisect_right(ends, k * cap) for k in range(len(pieces) + 1)], name
        assert bounds[-1] == n


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
