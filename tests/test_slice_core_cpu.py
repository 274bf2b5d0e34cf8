"""The predicates and the splice arithmetic of `sbx-slice` (sambamba_amd/csrc/slice_core.hpp), compiled for the host with g++ into
tests/native/slice_host.cpp -- once plainly, once under AddressSanitizer and UBSan.  The predicates are compared with loops over every
(ref, pos, cov, beg, end) of a small box (cov == 0 and pos == beg included); the splice arithmetic with a restatement in Python over
every (a, b) of a small block table, and by hand on each of its branches.  No GPU needed."""
import os
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "slice_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
TABLE = [0, 10, 25, 26, 40]         # four blocks, one of a single byte


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slicec") / "slice_host")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("slicec_san") / "slice_host_san")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def splice_ref(a, b, off):
    """(head_beg, head_end, blk0, blk1, tail_beg, tail_end): bytes of [a, b) not in a whole block go to head (a's block) or tail"""
    b = min(b, off[-1])
    if a >= b:
        return (a, a, 0, 0, a, a)
    whole = [k for k in range(len(off) - 1) if a <= off[k] and off[k + 1] <= b]
    ba = max(k for k in range(len(off) - 1) if off[k] <= a)
    head_end = a if a == off[ba] else min(b, off[ba + 1])
    if head_end == b:
        return (a, b, ba + 1, ba + 1, b, b)
    bb = len(off) - 1 if b == off[-1] else max(k for k in range(len(off) - 1) if off[k] <= b)
    blk0 = ba if a == off[ba] else ba + 1
    assert whole == list(range(blk0, bb))
    return (a, head_end, blk0, bb, off[bb], b)


def run_splice(exe, cases, off=TABLE):
    text = "".join("%d %s %d %d\n" % (len(off) - 1, " ".join(map(str, off)), a, b) for a, b in cases)
    r = subprocess.run([exe, "splice"], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return [tuple(int(x) for x in row.split()) for row in r.stdout.decode().splitlines()]


def test_predicates_against_brute_force(host, host_san):
    for exe in (host, host_san):
        r = subprocess.run([exe, "predicates"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 0, (r.stdout + r.stderr).decode()[-3000:]
        assert int(r.stdout) > 10000


def test_every_branch_of_the_splice_by_hand(host):
    cases = {
        "same block": ((3, 7), (3, 7, 1, 1, 7, 7)),
        "same block, a on its start": ((10, 20), (10, 10, 1, 1, 10, 20)),
        "a on a block start": ((10, 30), (10, 10, 1, 3, 26, 30)),
        "b on a block start": ((3, 25), (3, 10, 1, 2, 25, 25)),
        "head and tail both empty": ((10, 26), (10, 10, 1, 3, 26, 26)),
        "b at the end of the stream": ((12, 40), (12, 25, 2, 4, 40, 40)),
        "adjacent blocks, nothing copied": ((3, 15), (3, 10, 1, 1, 10, 15)),
        "one whole block between head and tail": ((12, 29), (12, 25, 2, 3, 26, 29)),
        "the one-byte block copied": ((24, 27), (24, 25, 2, 3, 26, 27)),
        "empty": ((30, 30), (30, 30, 0, 0, 30, 30)),
        "whole stream": ((0, 40), (0, 0, 0, 4, 40, 40)),
    }
    got = run_splice(host, [c for c, _ in cases.values()])
    for (name, (_, want)), g in zip(cases.items(), got):
        assert g == want, (name, g, want)


def test_splice_equals_the_restatement_everywhere(host, host_san):
    cases = [(a, b) for a in range(0, 41) for b in range(0, 43)]
    want = [splice_ref(a, b, TABLE) for a, b in cases]
    for exe in (host, host_san):
        assert run_splice(exe, cases) == want
    # every byte of [a, b) is in exactly one of head, blocks, tail
    for (a, b), (h0, h1, k0, k1, t0, t1) in zip(cases, want):
        b = min(b, 40)
        if a < b:
            assert (h1 - h0) + (TABLE[k1] - TABLE[k0]) + (t1 - t0) == b - a and h0 == a and t1 == b
