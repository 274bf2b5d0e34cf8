"""The validity of a record (sambamba_amd/csrc/valid_core.hpp), compiled for the host with g++ into tests/native/valid_host.cpp:
the hand-made records of tests/valid_cases.py against the masks written down there, the Python restatement (tests/valid_ref.py)
against the same masks, both on seeded random mutations of the cases and on every truncation of every case -- the latter with
guard bytes behind the record, and once more under AddressSanitizer and UBSan.  No GPU needed."""
import os
import random
import struct
import subprocess

import pytest

from tests import valid_cases as cases
from tests import valid_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "valid_host.cpp")
N_MUTATIONS = 4000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("validc") / "valid_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("validc_san") / "valid_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, mode, recs):
    data = "".join((r.hex() or "-") + "\n" for r in recs)
    r = subprocess.run([exe, mode], input=data.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    rows = [[int(x) for x in row.split()] for row in r.stdout.decode().splitlines()]
    assert len(rows) == len(recs)
    return rows


def names(m):
    return [c for k, c in enumerate(ref.CLASSES) if m >> k & 1]


def mutations(seed, n):
    """the cases with one to three bytes changed, a byte dropped or a byte doubled; block_size re-stamped half of the time"""
    rng = random.Random(seed)
    base = [r for _, r, _ in cases.cases()]
    interesting = [0, 1, 0x20, 0x21, 0x40, 0x5D, 0x5E, 0x7E, 0x7F, 0x80, 0xFF, ord("H"), ord("Z"), ord("B"), ord("A"), ord("i"), ord("^")]
    out = []
    for _ in range(n):
        r = bytearray(rng.choice(base))
        kind = rng.randrange(4)
        if kind < 2:
            for _ in range(rng.randrange(1, 4)):
                r[rng.randrange(4, len(r))] = rng.choice(interesting) if rng.random() < 0.7 else rng.randrange(256)
        elif kind == 2:
            del r[rng.randrange(4, len(r))]
        else:
            at = rng.randrange(4, len(r))
            r.insert(at, r[at])
        if kind >= 2 and rng.random() < 0.5:
            r[0:4] = struct.pack("<I", len(r) - 4)
        out.append(bytes(r))
    return out


def test_the_restatement_gives_the_masks_written_down():
    for label, r, want in cases.cases():
        assert names(ref.mask(r)) == names(want), label


def test_the_core_gives_the_masks_written_down(host):
    cs = cases.cases()
    assert len(cs) > 150 and sum(1 for _, _, m in cs if m == 0) > 50
    for (label, _, want), (got,) in zip(cs, run(host, "masks", [r for _, r, _ in cs])):
        assert names(got) == names(want), label
    # every class occurs, alone, in some case
    assert {m for _, _, m in cs} >= {1 << k for k in range(10)}


def test_core_and_restatement_agree_on_mutations(host):
    recs = mutations(20260101, N_MUTATIONS)
    got = [m for (m,) in run(host, "masks", recs)]
    want = [ref.mask(r) for r in recs]
    differ = [(r.hex(), names(g), names(w)) for r, g, w in zip(recs, got, want) if g != w]
    assert not differ, differ[:3]
    assert len({m for m in want}) > 20 and sum(1 for m in want if m == 0) > N_MUTATIONS // 20      # (the mutations reach the rules)


def test_every_truncation_of_every_case(host):
    recs = [r for _, r, _ in cases.cases() if len(r) < 400]
    for r, row in zip(recs, run(host, "cuts", recs)):
        assert row == [ref.mask(r[:n]) for n in range(len(r) + 1)]
        assert all(m == ref.MALFORMED for m in row[:min(len(r), 4 + struct.unpack_from("<I", r)[0])])      # a cut record is malformed, no more


def test_under_sanitizers(host_san):
    cs = cases.cases()
    recs = [r for _, r, _ in cs]
    assert [m for (m,) in run(host_san, "masks", recs)] == [m for _, _, m in cs]          # (a finding ends the program with a non-zero status)
    run(host_san, "cuts", [r for r in recs if len(r) < 400])
    # the same cuts with block_size stamped to the cut: the record is whole again and its tail is what gets cut
    stamped = []
    for r in recs:
        if 40 < len(r) < 400:
            stamped += [struct.pack("<I", n - 4) + r[4:n] for n in range(36, len(r))]
    assert len(stamped) > 4000
    got = [m for (m,) in run(host_san, "masks", stamped)]
    assert got == [ref.mask(r) for r in stamped]
    muts = mutations(7, 1500)
    assert [m for (m,) in run(host_san, "masks", muts)] == [ref.mask(r) for r in muts]
