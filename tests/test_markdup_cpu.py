"""`sambamba markdup` without a GPU: the restatement (tests/markdup_ref.py) against answers written down by hand, one scenario per
rule of markdup.d; the header text against literals; and sambamba_amd/csrc/markdup_core.hpp, compiled for the host with g++ into
tests/native/markdup_host.cpp, against the restatement -- 5' coordinate and score over a CIGAR grid, the packed keys against the
comparators, the header text."""
import itertools
import os
import struct
import subprocess

import pytest

from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests.flagstat_ref import inflate
from tests.util import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "native", "markdup_host.cpp")
FIXTURES = ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates")


# ---- known answers ------------------------------------------------------------------------------------------------------------
def test_scenarios_known_answers():
    records, dups, flags, counts = mc.scenarios()
    names = mc.labels(records)
    got, n_pairs, n_single, n_unmatched = ref.analyse(records, mc.TEXT)
    assert sorted(names[i] for i in got) == sorted(dups)
    assert (n_pairs, n_single, n_unmatched) == counts == (12, 23, 4)
    assert ref.duplicates(records, mc.TEXT) == got


def test_each_rule_on_its_own():
    """The same rules, each scenario alone (so that no rule hides behind another) -- the duplicate NAMES are literals."""
    r = mc.rec
    cases = [
        ([r("A", 0, 100, flag=mc.F1, qual=30), r("A", 0, 300, flag=mc.R2, qual=30), r("B", 0, 100, flag=mc.F1, qual=20), r("B", 0, 300, flag=mc.R2, qual=20)],
         ["B#0", "B#1"]),
        ([r("B", 0, 100, flag=mc.F1, qual=20), r("B", 0, 300, flag=mc.R2, qual=20), r("A", 0, 100, flag=mc.F1, qual=30), r("A", 0, 300, flag=mc.R2, qual=30)],
         ["B#0", "B#1"]),
        ([r("A", 0, 100, flag=mc.F1), r("A", 0, 300, flag=mc.R2), r("B", 0, 100, flag=mc.F1), r("B", 0, 300, flag=mc.R2)], ["B#0", "B#1"]),
        ([r("A", 0, 100, flag=mc.F1), r("A", 0, 300, flag=mc.R2), r("B", 0, 100, flag=0x41), r("B", 0, 310, flag=mc.F2)], []),
        ([r("A", 0, 100, flag=mc.F1), r("A", 0, 300, flag=mc.R2), r("B", 0, 100, flag=mc.F1), r("B", 0, 301, flag=mc.R2)], []),
        ([r("P", 0, 100, flag=mc.F1), r("P", 0, 300, flag=mc.R2), r("f", 0, 100, qual=40), r("g", 0, 300, flag=0x10, qual=40)], ["f#0", "g#0"]),
        ([r("a", 0, 100, qual=20), r("b", 0, 100, qual=30)], ["a#0"]),
        ([r("a", 0, 100, qual=30), r("b", 0, 100, qual=30), r("c", 0, 100, qual=30)], ["b#0", "c#0"]),
        ([r("a", 0, 100)], []),
        ([r("f", 0, 100, qual=40), r("u", 0, 100, flag=mc.F1, qual=20)], ["f#0"]),
        ([r("a", 0, 105, "5S10M"), r("b", 0, 103, "3H10M"), r("c", 0, 102, "1H1S10M", qual=20)], ["b#0", "c#0"]),
        ([r("a", 0, 100, "10M5S", flag=0x10, qual=20), r("b", 0, 105, "10M", flag=0x10, qual=35), r("c", 0, 101, "4M2D6M2H", flag=0x10, qual=20)],
         ["a#0", "c#0"]),
        ([r("a", 0, 100, rg="gA"), r("b", 0, 100, rg="gC")], []),
        ([r("a", 0, 100, rg="gA", qual=30), r("b", 0, 100, rg="gB", qual=20)], ["b#0"]),
        ([r("a", 0, 100, rg="zz", qual=30), r("b", 0, 100, qual=20)], ["b#0"]),
        ([r("n", 0, 100, flag=mc.F1, rg="gA"), r("n", 0, 300, flag=mc.R2, rg="gB"), r("m", 0, 100, flag=mc.F1, rg="gA"), r("m", 0, 300, flag=mc.R2, rg="gA"),
          r("o", 0, 100, flag=mc.F1, rg="gA", qual=20), r("o", 0, 300, flag=mc.R2, rg="gA", qual=20)], ["o#0", "o#1"]),
        ([r("t", 0, 100, flag=mc.F1), r("t", 0, 300, flag=mc.R2), r("t", 0, 100, flag=mc.F1), r("f", 0, 100, qual=40)], ["f#0"]),
        ([r("A", 1, 50, flag=0x41), r("A", 0, 400, flag=mc.F2), r("B", 0, 400, flag=0x41, qual=20), r("B", 1, 50, flag=mc.F2, qual=20)], ["B#0", "B#1"]),
    ]
    for records, want in cases:
        names = mc.labels(records)
        assert sorted(names[i] for i in ref.duplicates(records, mc.TEXT)) == sorted(want), names


def test_output_flags_and_order():
    from tests import bamgen
    records, dups, flags, _ = mc.scenarios()
    names = mc.labels(records)
    stream = bamgen.bam_header(mc.TEXT, mc.REFS) + b"".join(records)
    for remove in (False, True):
        out = ref.split_stream(ref.expected_stream(stream, remove=remove))[3]
        got = {}
        by_body = {r[:18] + r[20:]: n for r, n in zip(records, names)}
        order = []
        for o in out:
            n = by_body[o[:18] + o[20:]]
            got[n] = struct.unpack_from("<H", o, 18)[0]
            order.append(n)
        assert order == [n for n in names if n in got]                       # input order
        if remove:
            assert set(names) - set(got) == dups | {"s15s#0", "s15x#0"}      # the kept 0x400 of a secondary / supplementary record removes it too
        else:
            assert len(out) == len(records)
            assert {n for n, f in got.items() if f & 0x400} == dups | {"s15s#0", "s15x#0"}
            for n, f in flags.items():
                assert got[n] == f, n


def test_generator_marks_a_sensible_share():
    for seed, shuffled in ((1, False), (2, True)):
        records = mc.random_records(20000, seed, shuffled)
        dup, n_pairs, n_single, n_unmatched = ref.analyse(records, mc.TEXT)
        assert 0.05 * len(records) <= len(dup) <= 0.95 * len(records)
        assert n_pairs > 1000 and n_unmatched > 100 and n_single > n_unmatched


# ---- header ---------------------------------------------------------------------------------------------------------------------
SQ = "@SQ\tSN:c1\tLN:1000\n"
HEADERS = {
    "no_hd": (SQ, "markdup a b", "@HD\tVN:1.3\n" + SQ + "@PG\tID:sambamba\tCL:markdup a b\tVN:1.0\n"),
    "coordinate": ("@HD\tVN:1.6\tSO:coordinate\n" + SQ, "markdup a b", "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@PG\tID:sambamba\tCL:markdup a b\tVN:1.0\n"),
    "queryname": ("@HD\tVN:1.5\tSO:queryname\n" + SQ, "markdup -r a b", "@HD\tVN:1.5\tSO:queryname\n" + SQ + "@PG\tID:sambamba\tCL:markdup -r a b\tVN:1.0\n"),
    "unsorted": ("@HD\tVN:1.6\tSO:unsorted\n" + SQ, "markdup a b", "@HD\tVN:1.6\tSO:unsorted\n" + SQ + "@PG\tID:sambamba\tCL:markdup a b\tVN:1.0\n"),
    "bogus": ("@HD\tVN:1.6\tSO:bogus\n" + SQ, "markdup a b", "@HD\tVN:1.6\n" + SQ + "@PG\tID:sambamba\tCL:markdup a b\tVN:1.0\n"),
    "unknown": ("@HD\tVN:1.6\tSO:unknown\n" + SQ, "markdup a b", "@HD\tVN:1.6\n" + SQ + "@PG\tID:sambamba\tCL:markdup a b\tVN:1.0\n"),
    "no_so": ("@HD\tVN:1.6\n" + SQ, "markdup a b", "@HD\tVN:1.6\n" + SQ + "@PG\tID:sambamba\tCL:markdup a b\tVN:1.0\n"),
    "two_pg": ("@HD\tVN:1.6\n" + SQ + "@PG\tID:bwa\tPN:bwa\n@PG\tID:fix\tPP:bwa\n@CO\tc\n", "markdup a b",
               "@HD\tVN:1.6\n" + SQ + "@PG\tID:bwa\tPN:bwa\n@PG\tID:fix\tPP:bwa\n@PG\tID:sambamba\tCL:markdup a b\tPP:fix\tVN:1.0\n@CO\tc\n"),
    "has_sambamba": ("@HD\tVN:1.6\n" + SQ + "@PG\tID:sambamba\tCL:view x\n@PG\tID:z\n", "markdup a b",
                     "@HD\tVN:1.6\n" + SQ + "@PG\tID:sambamba\tCL:view x\n@PG\tID:z\n"),
    "no_command_line": ("@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@PG\tID:bwa\n", None, "@HD\tVN:1.6\tSO:coordinate\n" + SQ + "@PG\tID:bwa\n"),
    "hd_not_first": (SQ + "@HD\tVN:1.6\tSO:coordinate\n", None, "@HD\tVN:1.3\n" + SQ),
}


@pytest.mark.parametrize("name", sorted(HEADERS))
def test_header_text_known_answers(name):
    text, cl, want = HEADERS[name]
    assert ref.header_text(text, cl) == want


def test_library_ids():
    assert ref.library_ids(mc.TEXT) == {"gA": 0, "gB": 0, "gC": 1}
    assert ref.library_ids("@RG\tID:a\n@RG\tID:b\tLB:x\n@RG\tID:c\n@RG\tID:a\tLB:y\n") == {"a": 0, "b": 1, "c": 0}


# ---- markdup_core.hpp on the host -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mdc") / "markdup_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


def run(exe, args, data=b""):
    return subprocess.run([exe] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


CIGARS = ["", "10M", "3S10M", "3H10M", "2H3S10M", "10M4S", "10M4H", "10M4S2H", "3S10M4S", "1H2S4M1I2M3D4M2N1=1X5S1H", "5S", "5H", "2H5S3H",
          "4M2D4M", "4M2I4M", "4M7N4M", "4=3X", "2S4=3X1S", "3I", "1S3I1S"]
QUALS = [[], [0], [14], [15], [255], [0, 14, 15, 255, 40, 2], [255] * 300]


def test_coordinate_and_score_grid(host):
    from tests import bamgen
    grid = [(pos, rev, bamgen.parse_cigar(c), q) for pos in (0, 7, 100000, 2 ** 31 - 20) for rev in (0, 1) for c in CIGARS for q in QUALS[:2]]
    grid += [(50, rev, bamgen.parse_cigar("2S5M"), q) for rev in (0, 1) for q in QUALS]
    lines = "".join("%d %d %d %s %d %s\n" % (pos, rev, len(c), " ".join("%d %d" % ("MIDNSHP=X".index(op), n) for op, n in c), len(q),
                                             " ".join(map(str, q))) for pos, rev, c, q in grid)
    r = run(host, ["ends"], lines.encode())
    assert r.returncode == 0, r.stderr
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert got == [(ref.five_prime_coord(pos, rev, c), ref.score(q)) for pos, rev, c, q in grid]
    # and the restatement itself on answers worked out by hand
    pc = bamgen.parse_cigar
    assert ref.five_prime_coord(100, 0, pc("3S10M")) == 97 and ref.five_prime_coord(100, 0, pc("2H3S10M4S")) == 95
    assert ref.five_prime_coord(100, 1, pc("3S10M")) == 110 and ref.five_prime_coord(100, 1, pc("10M4S2H")) == 116
    assert ref.five_prime_coord(100, 1, pc("4M2D4M1I7N2=1X")) == 120 and ref.five_prime_coord(2, 0, pc("5S")) == -3
    assert ref.five_prime_coord(2, 1, pc("2H5S")) == 9 and ref.five_prime_coord(5, 0, []) == 5 and ref.five_prime_coord(5, 1, []) == 5
    assert ref.score([0, 14, 15, 255, 40, 2]) == 310 and ref.score([]) == 0


REF_BITS = 5
SINGLES = [(lib, rid, coord, rev) for lib in (-1, 0, 3) for rid in (0, 1, 24) for coord in (-2 ** 31, -5, 0, 7, 2 ** 31 - 1) for rev in (0, 1)]


def test_position_key_orders_as_the_comparator(host):
    r = run(host, ["poskeys", REF_BITS], "".join("%d %d %d %d\n" % s for s in SINGLES).encode())
    assert r.returncode == 0, r.stderr
    keys = [int(x) for x in r.stdout.split()]
    assert len(keys) == len(SINGLES) and len(set(keys)) == len(keys)
    for (a, ka), (b, kb) in itertools.product(zip(SINGLES, keys), repeat=2):
        assert (ka < kb) == ref.single_end_before(a, b), (a, b)


def test_pair_key_orders_as_the_comparator_and_swaps(host):
    ends = [(rid, coord, rev) for rid in (0, 2) for coord in (-3, 10) for rev in (0, 1)]
    grid = [(lib, a, b) for lib in (-1, 1) for a in ends for b in ends]
    lines = "".join("%d %d %d %d 100 %d %d %d 200\n" % ((lib,) + a + b) for lib, a, b in grid)
    r = run(host, ["pairkeys", REF_BITS], lines.encode())
    assert r.returncode == 0, r.stderr
    words = [tuple(int(x) for x in line.split()) for line in r.stdout.decode().splitlines()]
    assert len(words) == len(grid)

    def end(lib, e, score):
        return {"library": lib, "ref": e[0], "coord": e[1], "reversed": e[2], "score": score}
    want = [ref.combine(end(lib, a, 100), end(lib, b, 200)) for lib, a, b in grid]
    pos = {s: int(k) for s, k in zip(SINGLES, run(host, ["poskeys", REF_BITS], "".join("%d %d %d %d\n" % s for s in SINGLES).encode()).stdout.split())}
    for (w0, w1, w2, end2), (key, k1, k2, score) in zip(words, want):
        assert w2 == (~score) & 0xFFFFFFFF and score == 300
    for (wa, ka), (wb, kb) in itertools.product(zip(words, want), repeat=2):
        assert (wa[:2] < wb[:2]) == ref.paired_ends_before(ka[0], kb[0]), (ka, kb)
        assert (wa[:2] == wb[:2]) == (ka[0] == kb[0])
    # the marker of the second end is its position key; the swap took place when the later record is strictly smaller
    r2 = run(host, ["poskeys", REF_BITS], "".join("%d %d %d %d\n" % k2 for _, _, k2, _ in want).encode())
    assert [w[3] for w in words] == [int(x) for x in r2.stdout.split()]
    r1 = run(host, ["poskeys", REF_BITS], "".join("%d %d %d %d\n" % k1 for _, k1, _, _ in want).encode())
    assert [w[0] for w in words] == [int(x) for x in r1.stdout.split()]
    assert any(k1[1:] == b and a != b for (lib, a, b), (_, k1, _, _) in zip(grid, want))
    # a better score sorts first inside a group
    r3 = run(host, ["pairkeys", REF_BITS], b"0 0 5 0 10 0 9 1 10\n0 0 5 0 10 0 9 1 11\n0 0 5 0 4294967295 0 9 1 2\n")
    w = [tuple(int(x) for x in line.split()) for line in r3.stdout.decode().splitlines()]
    assert w[1][2] < w[0][2] and w[2][2] == (~1) & 0xFFFFFFFF


def test_key_fits(host):
    assert run(host, ["fits", 3, 25]).stdout.split() == [b"1", b"5"]
    assert run(host, ["fits", 0, 1]).stdout.split() == [b"1", b"0"]
    # 33 bits of coordinate and strand, 12 of 3366 references: 18 bits are left for library + 1
    assert run(host, ["fits", 2 ** 18 - 1, 3366]).stdout.split() == [b"1", b"12"]
    assert run(host, ["fits", 2 ** 18, 3366]).stdout.split()[0] == b"0"
    assert run(host, ["fits", 2 ** 29, 2 ** 20]).stdout.split()[0] == b"0"


def _bam_text(name):
    stream = inflate(os.path.join(GOLDEN, name + ".bam"))
    return stream[8:8 + struct.unpack_from("<i", stream, 4)[0]].decode()


@pytest.mark.parametrize("name", sorted(HEADERS))
def test_native_header_text(host, name):
    text, cl, want = HEADERS[name]
    r = run(host, ["header"] + ([cl] if cl is not None else []), text.encode())
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == want


@pytest.mark.parametrize("name", FIXTURES)
def test_native_header_text_of_the_fixtures(host, name):
    text = _bam_text(name)
    for cl in (None, "markdup in.bam out.bam"):
        r = run(host, ["header"] + ([cl] if cl is not None else []), text.encode())
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == ref.header_text(text, cl)
    assert run(host, ["header"], b"@HD\tVN:1.6\nnot a header line\n").returncode == 3


def test_header_text_through_the_library():
    import sambamba_amd
    for text, cl, want in HEADERS.values():
        assert sambamba_amd.markdup_header_text(text, cl) == want
    with pytest.raises(sambamba_amd.SbxError):
        sambamba_amd.markdup_header_text("junk line\n")


def test_sort_header_text_is_unchanged():
    """The serialiser markdup shares with sort still prints sort's header."""
    import sambamba_amd
    from tests import sort_ref
    for text, _, _ in HEADERS.values():
        assert sambamba_amd.sort_header_text(text) == sort_ref.header_text(text)
