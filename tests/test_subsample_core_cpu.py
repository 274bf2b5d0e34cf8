"""The arithmetic of `sbx-subsample` (sambamba_amd/csrc/subsample_core.hpp: counted or not, the span with its clips, the keep predicate,
the slots of the coverage array), compiled for the host with g++ into tests/native/subsample_host.cpp -- once plainly, once under
AddressSanitizer and UBSan -- and compared with tests/subsample_ref.py and with Python's integers.  Next to it the patch offset K21
gained for the flag (tests/native/stream_patch_host.cpp).  No GPU needed."""
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import subsample_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "subsample_host.cpp")
PATCH_SRC = os.path.join(ROOT, "tests", "native", "stream_patch_host.cpp")
FLAGS = ["-std=c++17", "-Wall"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("subsamplec")
    plain, san = str(d / "subsample_host"), str(d / "subsample_host_san")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", plain, SRC])
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + SAN + ["-o", san, SRC])
    return plain, san


def ask(exe, mode, lines):
    r = subprocess.run([exe, mode], input="".join(l + "\n" for l in lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    return r.stdout.decode().splitlines()


def test_keep_predicate_at_its_edges(hosts):
    cases = []
    for max_cov in (1, 5, 10, 1000, (1 << 31) - 1):
        bound = max_cov << 32
        for cov in (1, max_cov, max_cov + 1, 2 * max_cov + 1, 21, (1 << 32) - 17, (1 << 32) - 1):
            if cov >= 1 << 32:
                continue
            # h * cov one step below, at and above max_cov << 32, and the ends of the hash's range
            h0 = bound // cov
            for h in (0, 1, h0 - 1, h0, h0 + 1, (1 << 32) - 1):
                if 0 <= h < 1 << 32:
                    cases.append((h, cov, max_cov))
    # h * cov exactly one below, at and one above max_cov << 32
    edge = [(1431655765, 3, 1), (1 << 31, 6, 3), (2863311531, 3, 2)]
    assert [h * cov - (m << 32) for h, cov, m in edge] == [-1, 0, 1]
    cases += edge
    want = ["1" if cov <= m or h * cov < (m << 32) else "0" for h, cov, m in cases]
    assert want[-3:] == ["1", "0", "0"] and "0" in want[:-3] and "1" in want[:-3] and len(cases) > 150
    assert [ref.keeps(*c) for c in edge] == [True, False, False]
    for exe in hosts:
        assert ask(exe, "keeps", ["%d %d %d" % c for c in cases]) == want


def test_counted_and_span_clips_on_their_own(hosts):
    """values no generated record carries: a sum of bases near 2^32, a position near 2^31"""
    big = (1 << 31) - 1
    cases = [  # flag ref n_ref pos ln bases -> counted, e
        ((0, 0, 1, 0, 100, 50), "1 50"), ((0, 0, 1, 90, 100, 10), "1 100"), ((0, 0, 1, 90, 100, 11), "1 100"),
        ((0, 0, 1, 99, 100, 0), "1 100"), ((0, 0, 1, 99, 100, 1), "1 100"), ((0, 0, 1, 100, 100, 5), "0"), ((0, 0, 1, 101, 100, 5), "0"),
        ((0, 0, 1, 5, 100, 0), "1 6"), ((0, 0, 1, -1, 100, 5), "0"), ((0, -1, 1, 5, 100, 5), "0"), ((0, 1, 1, 5, 100, 5), "0"),
        ((0, 2, 3, 5, 100, 5), "1 10"), ((0, 3, 3, 5, 100, 5), "0"),
        ((4, 0, 1, 5, 100, 5), "0"), ((0x200, 0, 1, 5, 100, 5), "0"), ((0x400, 0, 1, 5, 100, 5), "0"), ((0x1 | 0x10 | 0x40 | 0x100 | 0x800, 0, 1, 5, 100, 5), "1 10"),
        ((0, 0, 1, big - 1, big, 0xFFFFFFFF), "1 %d" % big), ((0, 0, 1, big - 10, big, 1 << 31), "1 %d" % big),
        ((0, 0, 1, 5, big, 0xFFFFFFF0), "1 %d" % big), ((0, 0, 1, 0, 0, 1), "0"), ((0, 0, 1, 0, -5, 1), "0"),
    ]
    for exe in hosts:
        assert ask(exe, "parts", ["%d %d %d %d %d %d" % c for c, _ in cases]) == [w for _, w in cases]


def test_slot_offsets(hosts):
    tile = int(ask(hosts[0], "tile", [])[0])
    assert tile >= 1024 and tile % 1024 == 0
    for lns in ([1000], [10, 0, 7], [tile - 1], [tile], [tile - 1, tile, tile + 1], []):
        base = ref.slot_bases(lns)
        want = " ".join(map(str, base + [-(-base[-1] // tile)]))
        for exe in hosts:
            assert ask(exe, "slots", [" ".join(map(str, [len(lns)] + lns))]) == [want]
    assert ref.slot_bases([10, 0, 7]) == [0, 11, 12, 20]


def test_record_span_against_the_restatement(hosts):
    lns = [100, 0, 50]
    base = ref.slot_bases(lns)
    recs = []
    for ref_id in (-1, 0, 1, 2, 3):
        for pos in (-1, 0, 40, 49, 50, 98, 99, 100, 150):
            for cigar in ("", "1M", "10M", "5S10M5S", "3M2I3M", "3M2D3M1N1=1X", "60M", "5I", "4H"):
                for flag in (0, 0x10, 0x4, 0x200, 0x400, 0x404):
                    recs.append(bamgen.make_record(ref_id, pos, cigar, "ACGT", 30, name="n%d" % len(recs), flag=flag))
    broken = bytearray(bamgen.make_record(0, 5, "10M", "ACGT", 30, name="broken"))
    struct.pack_into("<H", broken, 16, 4000)             # a CIGAR count that runs past block_size
    recs.append(bytes(broken))
    noname = bytearray(bamgen.make_record(0, 5, "", "", [], name=""))
    recs.append(bytes(noname))
    want = []
    for rec in recs:
        l_name, n_cigar = rec[12], struct.unpack_from("<H", rec, 16)[0]
        if 32 + l_name + 4 * n_cigar > len(rec) - 4:
            want.append("bad")
            continue
        s = ref.span(rec, lns)
        name_len = max(l_name - 1, 0)
        want.append("uncounted %d" % name_len if s is None else
                    "counted %d %d %d %d" % (base[s[0]] + s[1], base[s[0]] + s[2], name_len, ref.flag_of(rec)))
    assert want.count("bad") == 1 and sum(w.startswith("counted") for w in want) > 100
    # every slot a counted record touches lies inside its own reference
    for rec, w in zip(recs, want):
        if w.startswith("counted"):
            r = struct.unpack_from("<i", rec, 4)[0]
            lo, hi = map(int, w.split()[1:3])
            assert base[r] <= lo < hi <= base[r + 1] - 1
    lines = ["%d %s %s" % (len(lns), " ".join(map(str, lns)), rec.hex()) for rec in recs]
    for exe in hosts:
        assert ask(exe, "span", lines) == want


def test_hash_is_fnv1a_with_a_zero_seed():
    """64-bit FNV-1a (published vectors), over the name and the eight zero bytes of the seed; the low half"""
    assert ref.fnv1a64(b"") == 0xCBF29CE484222325 and ref.fnv1a64(b"a") == 0xAF63DC4C8601EC8C and ref.fnv1a64(b"foobar") == 0x85944171F73967E8
    assert ref.name_hash32(b"read1") == ref.fnv1a64(b"read1" + bytes(8)) & 0xFFFFFFFF


def test_patch_offset_of_the_stream_plan(tmp_path):
    """K21's plan with the 16-bit patch at byte 18: window edges at dest + 17 .. dest + 20, under ASan + UBSan"""
    exe = str(tmp_path / "stream_patch_host")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + SAN + ["-o", exe, PATCH_SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    words = r.stdout.decode().split()
    assert words[0] == "cases" and int(words[1]) >= 2000 and words[2] == "split" and int(words[3]) >= 200
