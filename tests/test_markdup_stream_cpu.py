"""What the streamed path of sbx_markdup adds to sambamba_amd/csrc/markdup_core.hpp, without a GPU: the flag rule (flag_after / kept)
that K10d, the output plan and K10f share, and the entries of the key store K10b compares on that path (pair_key_len / pair_key_byte
/ pair_keys_equal).  tests/native/markdup_stream_host.cpp is compiled for the host with g++ twice -- plain, and under
-fsanitize=address,undefined -- and run as a program of its own; its answers are compared with the restatement's rule
(tests/markdup_ref.py) and with entries put together here."""
import os
import subprocess

import pytest

from tests import bamgen
from tests import markdup_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "markdup_stream_host.cpp")
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


@pytest.fixture(scope="module", params=sorted(BUILDS))
def host(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mdstream") / ("markdup_stream_host_" + request.param))
    subprocess.check_call(["g++", "-std=c++17", "-Wall"] + BUILDS[request.param] + ["-o", exe, SRC])
    return exe


def run(exe, mode, data=b""):
    r = subprocess.run([exe, mode], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_flag_rule_over_every_flag(host):
    """All 2^16 flags x dup x remove: the flag written is the restatement's output_flag, and a record is dropped exactly when -r is
    given and the flag WRITTEN carries 0x400 (expected_stream's rule)."""
    out = run(host, "flags")
    assert len(out) == 3 << 18
    want = bytearray()
    for flag in range(1 << 16):
        for dup in (False, True):
            f = ref.output_flag(flag, dup)
            for remove in (False, True):
                want += bytes((f & 0xFF, f >> 8, 0 if remove and f & 0x400 else 1))
    assert out == bytes(want)
    # and the rule itself on answers written down by hand
    assert ref.output_flag(0x400, False) == 0 and ref.output_flag(0x500, False) == 0x500 and ref.output_flag(0xC00, False) == 0xC00
    assert ref.output_flag(0x63, True) == 0x463 and ref.output_flag(0x100, True) == 0x500


def _record(name, rg, other=b""):
    """(record, rg_at, rg bytes or None): rg None -- no RG tag; `other` goes in front of the RG tag."""
    tags = bamgen.tag_i("NM", 3) + other + (bamgen.tag_z("RG", rg) if rg is not None else b"")
    rec = bamgen.make_record(0, 100, "4M", "ACGT", 30, name=name, flag=0x41, tags=tags)
    if rg is None:
        return rec, 0, None
    at = len(rec) - len(rg) - 1
    assert rec[at - 3:at] == b"RGZ" and rec[-1] == 0
    return rec, at, rg.encode()


def _entry(rec, rg):
    l_name = rec[12]
    return bytes((l_name,)) + rec[36:36 + l_name] + (rg or b"") + b"\0"


def test_entries_over_name_and_rg_lengths(host):
    """Names of 1 .. 254 characters x RG absent / empty / 300 characters: the entry is l_read_name, the name with its NUL, the RG
    value, NUL -- its length 2 + l_read_name + len(RG) -- and an absent RG gives the entry of an empty one."""
    cases = []
    for n in range(1, 255):
        name = "".join(chr(33 + (n * 7 + k) % 90) for k in range(n))
        for rg in (None, "", "g" * 299 + "X"):
            cases.append(_record(name, rg))
    lines = "".join("%s %d %d\n" % (rec.hex(), at, len(rg) if rg else 0) for rec, at, rg in cases)
    got = run(host, "keys", lines.encode()).decode().splitlines()
    assert len(got) == len(cases) == 254 * 3
    for (rec, at, rg), line in zip(cases, got):
        klen, hexed = line.split()
        want = _entry(rec, rg)
        assert int(klen) == len(want) == 2 + rec[12] + len(rg or b"")
        assert bytes.fromhex(hexed) == want
    assert got[0] == got[1] and got[0] != got[2]                    # absent == empty
    # a longer tag in front of RG moves rg_at, not the entry
    a, b = _record("n", "lane1"), _record("n", "lane1", other=bamgen.tag_z("XY", "filler"))
    assert b[1] == a[1] + 10
    out = run(host, "keys", ("%s %d 5\n%s %d 5\n" % (a[0].hex(), a[1], b[0].hex(), b[1])).encode()).decode().splitlines()
    assert out[0] == out[1]


def test_entry_equality(host):
    """pair_keys_equal is equality of the entries as byte strings -- which, with the length byte in front, is the resident
    comparison: same l_read_name, same name bytes, same RG string."""
    def e(name, rg, terminated=True):
        nm = name.encode() + (b"\0" if terminated else b"")
        return bytes((len(nm),)) + nm + rg.encode() + b"\0"
    entries = [e("a", ""), e("a", "x"), e("a", "xy"), e("ab", ""), e("ab", "c"), e("a", "bc"), e("b", ""), e("a" * 254, ""), e("a" * 254, "g"),
               e("a" * 253 + "b", ""), e("", ""), e("", "a"),
               # names without their NUL, and one with a NUL inside: name bytes and RG bytes change places, the length byte tells them apart
               e("ab", "", terminated=False), e("a", "b", terminated=False), e("a\0b", "", terminated=False), e("a", "b")]
    assert e("a\0b", "", False)[1:] == e("a", "b")[1:] and e("ab", "", False)[1:] == e("a", "b", False)[1:]
    pairs = [(p, q) for p in entries for q in entries]
    got = run(host, "equal", "".join("%s %s\n" % (p.hex(), q.hex()) for p, q in pairs).encode()).split()
    assert [int(x) for x in got] == [1 if p == q else 0 for p, q in pairs]
    assert sum(int(x) for x in got) == len(entries)                  # no two of them are equal


def test_abi_size_of_the_stream_stats():
    import ctypes as C
    import sambamba_amd
    from sambamba_amd._lib import MarkdupStreamStats
    assert sambamba_amd.lib().sbx_abi_sizeof(b"sbx_markdup_stream_stats") == C.sizeof(MarkdupStreamStats) == 4 * 4 + 3 * 8 + 5 * 8
    assert MarkdupStreamStats.struct_size.offset == 0 and MarkdupStreamStats.window_bytes.offset == 16
