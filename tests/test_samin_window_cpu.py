"""The part of a record that lies inside one window of the output stream (sampc::WindowSink, sam_record_emit_window of
sambamba_amd/csrc/samparse_core.hpp: what a lane of K15d runs for a record that straddles a window edge), compiled for the host with
g++ into tests/native/samin_window_host.cpp.  For every good line of tests/samin_cases.py and one line with 100,000 bases, and for
every cut c: the windows [0, c) and [c, length) joined are what sam_record_emit writes, the bytes reported are c and length - c,
the inner window [c, c + 8) holds its eight bytes, a record measured one byte short is an overrun that writes nothing outside the
clip, and no guard byte around any window changes.  Once plain, once under AddressSanitizer and UBSan.  No GPU needed.

The cuts: every c in [0, length] for a record of at most 4096 bytes.  Two records are longer -- the CIGAR of 65,535 operations
(262,189 bytes) and the 100,000-base line -- and four walks of such a line per cut make every cut a matter of minutes, so they take
the cuts at which the sink can go wrong: two bytes to either side of every field boundary (block_size, the fixed part, the name, the
CIGAR, SEQ, QUAL, every tag and every tag's value), every 8-byte group edge of SEQ and of QUAL counted from the field's start (every
16-byte edge is one of them), and a stride of 251 bytes -- a prime, so every residue of 4, 8 and 16 comes up -- through the whole
record.  The sanitizer build takes every 16th of the group edges."""
import os
import subprocess

import pytest

from tests import samin_cases as cases
from tests import samin_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "samin_window_host.cpp")
FLAGS = ["-std=c++17", "-Wall", "-pthread", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
ALL_CUTS_UP_TO = 4096
N_LONG = 100000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("saminw") / "samin_window_host")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("saminw_san") / "samin_window_host_san")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def long_line():
    seq = bytes(b"ACGTNacgtn=.RYKMSWBDHVrykmswbdhvXZxz"[k % 36] for k in range(N_LONG))
    qual = bytes(33 + (7 * k) % 94 for k in range(N_LONG))
    return cases.line(b"long100k", cigar=b"%dM" % N_LONG, seq=seq, qual=qual, tags=[b"NM:i:70000", b"XZ:Z:tail", b"XB:B:s,1,-2,3"])


def lines_under_test():
    g = dict(cases.good_lines())
    g["seq_100000"] = long_line()
    return g


def field_boundaries(line):
    """offsets in the record at which a field or a tag's value starts or ends, and (start, bytes) of SEQ and of QUAL"""
    f = line.split(b"\t")
    l_name = len(f[0]) + 1
    n_cigar = 0 if f[5] == b"*" else sum(1 for ch in f[5] if not 48 <= ch <= 57)
    l_seq = 0 if f[9] == b"*" else len(f[9])
    name_at, cigar_at = 36, 36 + l_name
    seq_at = cigar_at + 4 * n_cigar
    qual_at = seq_at + (l_seq + 1) // 2
    tags_at = qual_at + l_seq
    bounds = [0, 4, name_at, cigar_at, seq_at, qual_at, tags_at]
    # a tag ends where the record of the line without the tags behind it ends; its value starts three bytes in
    at = tags_at
    for k in range(11, len(f)):
        end = len(ref.record(b"\t".join(f[:k + 1]), cases.REF_NAMES))
        bounds += [at + 3, end]
        at = end
    assert at == len(ref.record(line, cases.REF_NAMES))
    return sorted(set(bounds)), (seq_at, (l_seq + 1) // 2), (qual_at, l_seq)


def cuts_of(line, edge_step=1):
    """"all", or the cuts of a long record (see the module's docstring) as a sorted list"""
    length = len(ref.record(line, cases.REF_NAMES))
    if length <= ALL_CUTS_UP_TO:
        return "all", length + 1
    bounds, (seq_at, seq_bytes), (qual_at, qual_bytes) = field_boundaries(line)
    cuts = set(range(0, length + 1, 251))
    for b in bounds:
        cuts.update(range(max(0, b - 2), min(length, b + 2) + 1))
    cuts.update(range(seq_at, seq_at + seq_bytes + 1, 8 * edge_step))
    cuts.update(range(qual_at, qual_at + qual_bytes + 1, 8 * edge_step))
    cuts = sorted(cuts)
    return " ".join(map(str, cuts)), len(cuts)


def run(exe, lines, edge_step=1):
    """[(status, length, cuts, failures, first failure)] of samin_window_host, and the number of cuts asked for per line"""
    asked = [cuts_of(l, edge_step) for l in lines]
    data = " ".join(n.encode().hex() for n in cases.REF_NAMES) + "\n" + "".join(l.hex() + "\n" + c + "\n" for l, (c, _) in zip(lines, asked))
    r = subprocess.run([exe], input=data.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = []
    for row in r.stdout.decode().splitlines():
        st, length, cuts, failures, first = row.split()
        out.append((int(st), int(length), int(cuts), int(failures), first))
    assert len(out) == len(lines)
    return out, [n for _, n in asked]


def check(exe, edge_step):
    g = lines_under_test()
    out, asked = run(exe, list(g.values()), edge_step)
    for name, (st, length, cuts, failures, first), n in zip(g, out, asked):
        assert st == 0 and length == len(ref.record(g[name], cases.REF_NAMES)), name
        assert cuts == n and failures == 0, (name, failures, first)
    return dict(zip(g, asked))


def test_the_long_records_take_the_listed_cuts():
    g = lines_under_test()
    long_names = [n for n, l in g.items() if cuts_of(l)[0] != "all"]
    assert long_names == ["cigar_65535", "seq_100000"]
    bounds, (seq_at, seq_bytes), (qual_at, qual_bytes) = field_boundaries(g["seq_100000"])
    assert (seq_bytes, qual_bytes) == (N_LONG // 2, N_LONG) and seq_at == 36 + 9 + 4 and qual_at == seq_at + seq_bytes
    cuts = set(map(int, cuts_of(g["seq_100000"])[0].split()))
    # every field boundary, every group edge of 8 and of 16 bytes in SEQ and QUAL, both ends of the record
    assert {0, 4, 36, 45, seq_at, qual_at, qual_at + qual_bytes} <= set(bounds) and len(bounds) == 7 + 2 * 3
    length = len(ref.record(g["seq_100000"], cases.REF_NAMES))
    assert all(b + d in cuts for b in bounds for d in (-2, -1, 0, 1, 2) if 0 <= b + d <= length)
    assert all(seq_at + k in cuts for k in range(0, seq_bytes + 1, 8)) and all(qual_at + k in cuts for k in range(0, qual_bytes + 1, 8))
    assert max(cuts) == length == bounds[-1]


def test_windows_join_to_the_record(host):
    asked = check(host, 1)
    assert asked["plain"] == len(ref.record(cases.line(), cases.REF_NAMES)) + 1 and asked["seq_100000"] > 18000


def test_under_sanitizers(host_san):
    check(host_san, 16)                                   # (a finding ends the program with a non-zero status)
