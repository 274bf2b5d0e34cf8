"""The arithmetic of `sambamba view`'s selection (sambamba_amd/csrc/view_core.hpp), compiled for the host with g++ into
tests/native/view_host.cpp and checked against the Python restatement (tests/view_ref.py): the overlap predicate of the reference's
random access, the subsampling hash and threshold, the flag test and parser of --num-filter, and the text of -I -- no GPU needed."""
import itertools
import os
import subprocess

import pytest

from tests import view_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "view_host.cpp")
STAR = 0xFFFFFFFF


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("viewc") / "view_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


def run(exe, args, data=b""):
    return subprocess.run([exe] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def test_overlap_predicate(host):
    start, end = 100, 110
    cases = [(ref_id, pos, cov) for ref_id in (3, 2, -1) for pos in (start - 2, start - 1, start, start + 1, end - 1, end) for cov in (0, 1, 2)]
    lines = "".join("%d %d %d 3 %d %d\n" % (r, p, c, start, end) for r, p, c in cases)
    r = run(host, ["overlap"], lines.encode())
    assert r.returncode == 0, r.stderr
    got = [int(x) for x in r.stdout.split()]
    assert got == [int(ref.overlaps(r_, p, c, (3, start, end))) for r_, p, c in cases]
    table = dict(zip(cases, got))
    # the two cases the issue names, and the rest of the table written out for the reference id that matches
    assert table[(3, start + 1, 0)] == 1          # covers nothing, strictly inside: selected
    assert table[(3, start, 0)] == 0              # covers nothing, at the start: not selected
    want = {(start - 2, 0): 0, (start - 2, 1): 0, (start - 2, 2): 0, (start - 1, 0): 0, (start - 1, 1): 0, (start - 1, 2): 1,
            (start, 0): 0, (start, 1): 1, (start, 2): 1, (start + 1, 0): 1, (start + 1, 1): 1, (start + 1, 2): 1,
            (end - 1, 0): 1, (end - 1, 1): 1, (end - 1, 2): 1, (end, 0): 0, (end, 1): 0, (end, 2): 0}
    assert {(p, c): v for (r_, p, c), v in table.items() if r_ == 3} == want
    assert not any(v for (r_, _, _), v in table.items() if r_ != 3)


def test_overlap_with_the_unmapped_region_and_negative_positions(host):
    cases = [(-1, -1, 0), (-1, 5, 0), (0, 5, 3), (7, -1, 0)]
    r = run(host, ["overlap"], "".join("%d %d %d %d 0 0\n" % (a, b, c, STAR) for a, b, c in cases).encode())
    assert [int(x) for x in r.stdout.split()] == [1, 1, 0, 0] == [int(ref.overlaps(a, b, c, "*")) for a, b, c in cases]
    # a record at position -1 that covers two bases reaches position 0: it overlaps [0, 10) only through what it covers
    r = run(host, ["overlap"], b"0 -1 2 0 0 10\n0 -1 1 0 0 10\n0 -1 0 0 0 10\n")
    assert [int(x) for x in r.stdout.split()] == [1, 0, 0]


@pytest.mark.parametrize("seed", [0, 1, 2 ** 63 + 5, 2 ** 64 - 1])
def test_hash_is_fnv1a_over_name_and_seed(host, seed):
    names = [b"", b"r", b"read/1", bytes(range(1, 255)), b"q" * 254]
    assert len(names[3]) == 254
    data = "".join((n.hex() or "-") + "\n" for n in names).encode()
    r = run(host, ["hash", seed], data)
    assert r.returncode == 0, r.stderr
    assert [int(x) for x in r.stdout.split()] == [ref.name_hash(n, seed) for n in names]


def test_hash_known_answers(host):
    # computed by hand from the definition (offset 14695981039346656037, prime 1099511628211, modulo 2^64)
    r = run(host, ["hash", 1], b"read/1".hex().encode() + b"\n")
    assert int(r.stdout) == 4192347811698619164
    r = run(host, ["hash", 0], b"-\n")
    assert int(r.stdout) == 12161962213042174405


def test_threshold(host):
    want = {"0": 0, "0.25": 1 << 30, "0.5": 1 << 31, "1.0": 1 << 32, "1.5": 3 << 31, "1e-10": 0}
    for text, value in want.items():
        r = run(host, ["threshold", text])
        assert (r.returncode, int(r.stdout)) == (0, value), text
        assert ref.threshold(float(text)) == value
    for text in ("-0.5", "nan", "-1e-30", "1e30"):
        assert run(host, ["threshold", text]).returncode == 3, text
        assert ref.threshold(float(text)) is None


def test_num_filter_parser(host):
    want = {"4/": (4, 0), "/4": (0, 4), "3": (3, 0), "": (0, 0), "3/1024": (3, 1024), "65535/0": (65535, 0), "/": (0, 0), "1/2/x": (1, 2)}
    for text, value in want.items():
        r = run(host, ["numfilter", text])
        assert r.returncode == 0, text
        assert tuple(int(x) for x in r.stdout.split()) == value == ref.num_filter(text), text
    for text in ("65536", "-1", "a/b", "4/65536", "1 /2", "+3", "0x10"):
        assert run(host, ["numfilter", text]).returncode == 3, text
        assert ref.num_filter(text) is None, text


def test_flag_test(host):
    cases = list(itertools.product((0, 4, 3, 0x403, 0xFFFF), (0, 4, 3), (0, 1024, 4)))
    r = run(host, ["flags"], "".join("%d %d %d\n" % c for c in cases).encode())
    assert [int(x) for x in r.stdout.split()] == [int(ref.flags_pass(*c)) for c in cases]


def test_reference_info_json(host):
    def text(refs):
        args = []
        for name, length in refs:
            args += [name.encode().hex() or "-", length]
        r = run(host, ["json"] + args)
        assert r.returncode == 0
        return r.stdout.decode()

    assert text([]) == "[]\n" == ref.reference_info_json([])
    # the quote sits in front of the brace: that is what the reference's code prints
    assert text([("chr1", 1000)]) == '["{name":"chr1","length":1000}]\n' == ref.reference_info_json([("chr1", 1000)])
    odd = 'a"b\\c\td?e/f'
    two = [("chr1", 1000), (odd, 2 ** 31 - 1)]
    assert text(two) == '["{name":"chr1","length":1000},"{name":"a\\"b\\\\c\\td\\/e/f","length":2147483647}]\n' == ref.reference_info_json(two)
