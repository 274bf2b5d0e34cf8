"""The SAM line of a record (sambamba_amd/csrc/sam_core.hpp), compiled for the host with g++ into tests/native/sam_host.cpp: %g of
floats against the C library's snprintf, and the lines of the edge-case records (tests/sam_cases.py) against the Python restatement
(tests/sam_ref.py) -- lengths, bytes, guards around the output, and once more under AddressSanitizer and UBSan.  No GPU needed."""
import os
import struct
import subprocess

import pytest

from tests import sam_cases as cases
from tests import sam_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "sam_host.cpp")
N_RANDOM = 2000000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samc") / "sam_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("samc_san") / "sam_host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def lines(exe, recs, ref_names=cases.REF_NAMES):
    """[(status, length, emit status, guards, line bytes)] of sam_host lines"""
    data = (" ".join(n.encode().hex() for n in ref_names) or "-") + "\n" + "".join(r.hex() + "\n" for r in recs)
    r = subprocess.run([exe, "lines"], input=data.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = []
    for row in r.stdout.decode().splitlines():
        st, length, est, guards, hx = row.split()
        out.append((int(st), int(length), int(est), int(guards), b"" if hx == "-" else bytes.fromhex(hx)))
    assert len(out) == len(recs)
    return out


def test_g_equals_snprintf(host):
    r = subprocess.run([host, "g", "20240611", str(N_RANDOM)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(r.stdout.decode()[-3000:])
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    checked = int(r.stdout.decode().split()[-3])
    assert checked > N_RANDOM + 256 * 2 * 68 + 21 * 9999 * 10 and r.stdout.decode().split()[-1] == "0"


def test_g_known_values(host):
    # the restatement's own %g against texts written out by hand
    bits = lambda v: struct.unpack("<I", struct.pack("<f", v))[0]
    want = [(0.0, "0"), (-0.0, "-0"), (1e-5, "1e-05"), (123456.5, "123456"), (1234567.0, "1.23457e+06"), (3.4028235e38, "3.40282e+38"),
            (1e-45, "1.4013e-45"), (float("inf"), "inf"), (-float("inf"), "-inf"), (0.0001, "0.0001"), (100000.0, "100000"), (999999.5, "1e+06"),
            (0.5, "0.5"), (1.0, "1")]
    for v, text in want:
        assert ref.fmt_g(bits(v)) == text
    assert ref.fmt_g(0x7FC00000) == "nan" and ref.fmt_g(0xFFC00000) == "-nan"
    rec = cases.raw_record(tags=b"".join(b"x%df" % (k % 10) + struct.pack("<f", v) for k, (v, _) in enumerate(want)) +
                           b"n0f\x00\x00\xc0\x7fn1f\x00\x00\xc0\xff")
    (st, length, est, guards, line), = lines(host, [rec])
    assert (st, est, guards) == (0, 0, 1)
    assert line.decode().rstrip("\n").split("\t")[11:] == ["x%d:f:%s" % (k % 10, t) for k, (_, t) in enumerate(want)] + ["n0:f:nan", "n1:f:-nan"]


@pytest.mark.parametrize("which", ["edge", "tags"])
def test_lines_equal_the_restatement(host, which):
    recs = cases.edge_records() if which == "edge" else cases.tag_records()
    for rec, (st, length, est, guards, line) in zip(recs, lines(host, recs)):
        want = ref.sam_line(rec, cases.REF_NAMES)
        assert st == 0 and est == 0 and guards == 1
        assert length == len(want) == len(line)           # sam_line_length equals the bytes emitted
        assert line == want, (line[:200], want[:200])


def test_a_few_lines_written_out(host):
    recs = cases.edge_records()
    by_name = {l.split(b"\t")[0]: l for _, _, _, _, l in lines(host, recs)}
    assert by_name[b"seq000"] == b"seq000\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*\n"
    assert by_name[b"seq002"] == b"seq002\t4\t*\t0\t0\t*\t*\t0\t0\tAG\t!(\n"
    assert by_name[b"pos0"] == b"pos0\t4\t*\t0\t0\t*\t*\t0\t-2147483648\tAG\t??\n"
    assert by_name[b"pos2"] == b"pos2\t4\t*\t-2147483648\t0\t*\t*\t-2147483648\t2147483647\tAG\t??\n"
    assert by_name[b"cigops"].split(b"\t")[5] == b"1M2I3D4N5S6H7P8=9X10?11?12?13?14?15?16?"
    assert by_name[b"ciglong"].split(b"\t")[5] == b"268435455S1M"
    assert by_name[b"qstar"].rstrip(b"\n").split(b"\t")[10] == b"*" and b" " in by_name[b"qlate"].split(b"\t")[10]
    assert [by_name[b"mate%d" % k].split(b"\t")[2:7:4] for k in range(5)] == [[b"*", b"*"], [b"c1", b"*"], [b"c2", b"="],
                                                                               [b"c1", b"chrWithALongerName_3"], [b"*", b"c2"]]
    assert by_name[b""].startswith(b"\t4\t*")              # l_read_name 0 and 1: the empty name


def test_malformed_records_are_told_not_read_on(host):
    bad = cases.malformed_records()
    out = lines(host, list(bad.values()))
    for name, (st, _, _, _, _) in zip(bad, out):
        assert st == 1, name
        with pytest.raises(ref.Malformed):
            ref.sam_line(bad[name], cases.REF_NAMES)
    # every truncation of a record with every kind of tag is either a line or "bad"
    full = cases.tag_records()[0]
    body = full[4:]
    cuts = [struct.pack("<i", n) + body[:n] for n in list(range(0, 120)) + list(range(len(body) - 40, len(body)))]
    for rec, (st, length, est, guards, line) in zip(cuts, lines(host, cuts)):
        try:
            want = ref.sam_line(rec, cases.REF_NAMES)
        except ref.Malformed:
            want = None
        assert (st == 1) == (want is None)
        assert want is None or (line == want and guards == 1 and est == 0)


def test_under_sanitizers(host_san):
    bad = cases.malformed_records()
    recs = cases.edge_records() + cases.tag_records() + list(bad.values())
    full = cases.tag_records()[0]
    recs += [struct.pack("<i", n) + full[4:4 + n] for n in range(0, len(full) - 4, 7)]
    out = lines(host_san, recs)                            # (a finding ends the program with a non-zero status)
    n_good = len(recs) - len(bad) - len(range(0, len(full) - 4, 7))
    assert all(st == 0 and g == 1 for st, _, _, g, _ in out[:n_good])
    r = subprocess.run([host_san, "g", "7", "20000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
