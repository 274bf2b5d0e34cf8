"""The chunk-and-carry logic of `index -F` (sambamba_amd/csrc/fasta_core.hpp) and the bin a record should carry (bins_core.hpp),
compiled for the host with g++ into tests/native/fasta_host.cpp -- once plainly, once under AddressSanitizer and UBSan -- against the
Python restatement tests/fai_ref.py: the reference's own fixture and its expected text, the edge texts, 300 seeded random texts,
every one at chunk sizes 16, 32, 48, 4096 and whole; the three refusals; reg2bin on the edges of every level.  No GPU needed."""
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import fai_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "fasta_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "test.fasta")
FLAGS = ["-std=c++17", "-Wall", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
CHUNKS = (16, 32, 48, 4096, 0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastac") / "fasta_host")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fastac_san") / "fasta_host_san")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, mode, text):
    r = subprocess.run([exe, mode], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines()


def index_all(exe, texts):
    """[{chunk size: ("ok", fai) | ("seq",) | ("bare", count, first)}] of the texts"""
    rows = run(exe, "fai", "".join((t.hex() or "-") + "\n" for t in texts))
    assert len(rows) == len(texts) * len(CHUNKS)
    out = [dict() for _ in texts]
    for row in rows:
        w = row.split()
        if w[2] == "ok":
            got = ("ok", b"" if w[3] == "-" else bytes.fromhex(w[3]))
        elif w[2] == "seq":
            got = ("seq",)
        else:
            got = ("bare", int(w[3]), int(w[4]))
        out[int(w[0])][int(w[1])] = got
    return out


def check(exe, named):
    names, texts = list(named), list(named.values())
    for name, text, got in zip(names, texts, index_all(exe, texts)):
        want = ref.expected(text)
        assert sorted(got) == sorted(CHUNKS), name
        for chunk in CHUNKS:
            assert got[chunk] == want, (name, chunk, got[chunk], want)


def test_restatement_on_the_golden_file_and_by_hand():
    data = open(GOLDEN, "rb").read()
    assert len(data) == 127
    assert ref.fai(data) == ref.GOLDEN_FAI
    assert ref.fai(ref.CASES["crlf"]) == b"a\t3\t4\t2\t4\n"
    assert ref.fai(ref.CASES["last_line_open"]) == b"a\t6\t3\t4\t5\n"
    assert ref.fai(ref.CASES["last_line_open_header"]) == b"a\t4\t3\t4\t5\nb\t0\t13\t0\t1\n"
    assert ref.fai(ref.CASES["empty_first_sequence_line"]) == b"a\t6\t3\t4\t5\n"
    assert ref.fai(ref.CASES["empty_name"]) == b"\t4\t2\t4\t5\n" == ref.fai(ref.CASES["empty_name_space"]).replace(b"\t4\t4\t", b"\t4\t2\t")
    assert ref.fai(ref.CASES["tab_in_header"]) == b"a\tb\t4\t7\t4\t5\n"
    assert ref.fai(ref.CASES["cr_in_lf_file"]) == b"a\t9\t3\t5\t6\n"
    assert ref.fai(ref.CASES["crlf_open_end_cr"]) == b"a\t5\t4\t2\t4\n"
    assert ref.fai(b"") == b""
    assert ref.expected(ref.ERRORS["sequence_first"]) == ("seq",) == ref.expected(ref.ERRORS["blank_first"])
    assert ref.expected(ref.ERRORS["bare_newline"]) == ("bare", 4, 2)
    assert ref.expected(ref.ERRORS["bare_newline_one"]) == ("bare", 1, 3)
    assert ref.CASES["cr_at_chunk_end"][15:17] == b"\r\n"


def test_golden_file_at_every_chunk_size(host):
    got = index_all(host, [open(GOLDEN, "rb").read()])[0]
    assert all(got[c] == ("ok", ref.GOLDEN_FAI) for c in CHUNKS), got


def test_edge_texts_equal_the_restatement(host):
    check(host, ref.CASES)


def test_refusals(host):
    check(host, ref.ERRORS)


def test_random_texts_equal_the_restatement(host):
    texts = ref.random_cases()
    assert len(texts) == 300
    kinds = [ref.expected(t)[0] for t in texts]
    assert kinds.count("ok") > 200
    check(host, {"random %d" % k: t for k, t in enumerate(texts)})


def test_under_sanitizers(host_san):
    named = dict(ref.CASES)
    named.update(ref.ERRORS)
    named["golden"] = open(GOLDEN, "rb").read()
    named.update({"random %d" % k: t for k, t in enumerate(ref.random_cases(n=100))})
    check(host_san, named)                                  # (a finding ends the program with a non-zero status)
    assert run(host_san, "reg2bin", "-1 -1\n0 1\n")[0] == "4680"


# ---- bins ----
def edge_intervals():
    out = [(-1, -1), (-1, 0), (0, 0), (0, 1), ((1 << 29) - 2, (1 << 29) - 2), ((1 << 29) - 2, (1 << 29) - 1), ((1 << 29) - 2, 1 << 29), (0, 1 << 29)]
    for shift in (14, 17, 20, 23, 26):
        b = 3 << shift                                      # a boundary of this level that is none of the next
        for beg in (b - 2, b - 1, b, b + 1):
            for span in (0, 1, 2, 3, (1 << shift) - 1, 1 << shift, (1 << shift) + 1):
                out.append((beg, beg + span))
    return out


def test_reg2bin_against_bamgen_on_the_level_edges(host):
    cases = edge_intervals()
    got = [int(x) for x in run(host, "reg2bin", "".join("%d %d\n" % c for c in cases))]
    assert got == [bamgen.reg2bin(b, e) for b, e in cases]
    assert got[0] == 4680 and got[3] == 4681
    assert {0, 1, 9, 73, 585, 4681} <= {g if g == 0 else max(f for f in (1, 9, 73, 585, 4681) if f <= g) for g in got}      # every level is met


def test_expected_bin_of_records(host, host_san):
    """binc::expected_bin: basesCovered() is 0 for a read flagged unmapped, M D N = X add up, I S H P do not; a CIGAR that runs past the
    record is refused"""
    def rec(ref, pos, cigar, flag=0):
        return bamgen.make_record(ref, pos, cigar, "ACGT", 30, name="read", flag=flag)

    recs = [
        (rec(0, 100, "50M"), bamgen.reg2bin(100, 150)),
        (rec(0, 16380, "2S3M1I2D1=1X5H"), bamgen.reg2bin(16380, 16387)),
        (rec(0, 16380, "4M"), bamgen.reg2bin(16380, 16384)),
        (rec(0, 1000, "3M%dN3M" % (1 << 27)), 0),
        (rec(0, 70000, ""), bamgen.reg2bin(70000, 70001)),
        (rec(0, 70000, "5I3S"), bamgen.reg2bin(70000, 70001)),
        (rec(0, 70000, "40000M", flag=0x4), bamgen.reg2bin(70000, 70001)),
        (rec(-1, -1, "", flag=0x4), 4680),
        (rec(1, -1, "5M"), 0),                               # [-1, 4) straddles every level
    ]
    rows = "".join(r.hex() + "\n" for r, _ in recs)
    short = bytearray(recs[1][0])
    struct.pack_into("<i", short, 0, 32 + short[12] + 4)    # block_size ends inside the CIGAR
    rows += bytes(short[:4 + 32 + short[12] + 4]).hex() + "\n"
    for exe in (host, host_san):
        out = run(exe, "records", rows)
        assert [int(o.split()[1]) for o in out[:-1]] == [want for _, want in recs], out
        assert out[-1] == "bad"
