"""A SAM line turned into a BAM record (sambamba_amd/csrc/samparse_core.hpp), compiled for the host with g++ into
tests/native/samin_host.cpp: the float parser against the C library's strtof, the records of the edge lines (tests/samin_cases.py)
against the Python restatement (tests/samin_ref.py) -- lengths, bytes, guards around the output, the malformed verdicts -- once more
under AddressSanitizer and UBSan, the bin against the .bai reader's bin code, and the golden SAM files through the restatement and
back through the SAM writer's restatement (tests/sam_ref.py).  No GPU needed."""
import os
import subprocess

import pytest

from tests import sam_ref
from tests import samin_cases as cases
from tests import samin_ref as ref
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "samin_host.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLAGS = ["-std=c++17", "-Wall", "-pthread", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__"]
N_LONG = 20000


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("saminc") / "samin_host")
    subprocess.check_call(["g++", "-O2"] + FLAGS + ["-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def host_san(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("saminc_san") / "samin_host_san")
    subprocess.check_call(["g++", "-O1", "-g"] + FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def records(exe, lines, ref_names=cases.REF_NAMES):
    """[(status, length, emit status, guards, record bytes)] of samin_host lines"""
    data = (" ".join(n.encode().hex() for n in ref_names) or "-") + "\n" + "".join(l.hex() + "\n" for l in lines)
    r = subprocess.run([exe, "lines"], input=data.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = []
    for row in r.stdout.decode().splitlines():
        st, length, est, guards, hx = row.split()
        out.append((int(st), int(length), int(est), int(guards), b"" if hx == "-" else bytes.fromhex(hx)))
    assert len(out) == len(lines)
    return out


def test_floats_equal_strtof(host):
    r = subprocess.run([host, "floats", "20241018", str(N_LONG)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    print(r.stdout.decode()[-3000:])
    assert r.returncode == 0, r.stdout.decode()[-3000:]
    words = r.stdout.decode().split()
    # 900,000 significands without a trailing zero, 84 exponents, two signs; then at least four literals per long round
    assert int(words[-3]) >= 900000 * 84 * 2 + 4 * N_LONG and words[-1] == "0"


def test_float_restatement_on_known_values():
    want = [(b"1", 0x3F800000), (b"-0", 0x80000000), (b".5", 0x3F000000), (b"0.1", 0x3DCCCCCD), (b"1e39", 0x7F800000), (b"-1e39", 0xFF800000),
            (b"1e-46", 0), (b"1e-45", 1), (b"3.4028235e38", 0x7F7FFFFF), (b"3.4028236e38", 0x7F800000), (b"16777217", 0x4B800000),
            (b"16777217.0000000000000000000001", 0x4B800001), (b"16777219", 0x4B800002), (b"inf", 0x7F800000), (b"+inf", 0x7F800000),
            (b"-inf", 0xFF800000), (b"nan", 0x7FC00000), (b"-nan", 0xFFC00000), (b"7.006492321624085e-46", 0), (b"7.006492321624086e-46", 1)]
    for text, bits in want:
        assert ref.float_bits(text) == bits, text
    for text in (b"1.", b"+nan", b"INF", b"1e", b"", b"e5", b"--1"):
        with pytest.raises(ref.Malformed):
            ref.float_bits(text)


def test_records_equal_the_restatement(host):
    good = cases.good_lines()
    for name, (st, length, est, guards, rec) in zip(good, records(host, list(good.values()))):
        want = ref.record(good[name], cases.REF_NAMES)
        assert st == 0 and est == 0 and guards == 1, name
        assert length == len(want) == len(rec), name          # sam_record_length equals the bytes emitted
        assert rec == want, (name, rec[:120], want[:120])


def test_a_few_records_written_out():
    good = cases.good_lines()
    for name, rec in cases.HAND.items():
        assert ref.record(good[name], cases.REF_NAMES) == rec, name


def test_malformed_lines_are_told(host):
    bad = cases.malformed_lines()
    for name, (st, _, _, _, _) in zip(bad, records(host, list(bad.values()))):
        assert st == 1, name
        with pytest.raises(ref.Malformed):
            ref.record(bad[name], cases.REF_NAMES)
    # no reference table at all: unmapped lines parse, a named reference does not
    good = cases.good_lines()
    (a, b) = records(host, [good["unmapped"], good["plain"]], ref_names=[])
    assert a[0] == 0 and a[4] == ref.record(good["unmapped"], []) and b[0] == 1
    # every truncation of a line with tags is a record or "bad", as the restatement says
    full = good["hand"]
    cuts = [full[:n] for n in range(len(full))]
    for text, (st, length, est, guards, rec) in zip(cuts, records(host, cuts)):
        try:
            want = ref.record(text, cases.REF_NAMES)
        except ref.Malformed:
            want = None
        assert (st == 1) == (want is None), text
        assert want is None or (rec == want and guards == 1 and est == 0)


def test_under_sanitizers(host_san):
    good, bad = cases.good_lines(), cases.malformed_lines()
    full = good["tag_B_borders"]
    lines = list(good.values()) + list(bad.values()) + [full[:n] for n in range(0, len(full), 3)]
    out = records(host_san, lines)                         # (a finding ends the program with a non-zero status)
    assert all(st == 0 and g == 1 for st, _, _, g, _ in out[:len(good)])
    assert all(st == 1 for st, _, _, _, _ in out[len(good):len(good) + len(bad)])
    r = subprocess.run([host_san, "bins", "7", "20000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])


def test_bin_against_the_bai_reader(host):
    r = subprocess.run([host, "bins", "20241018", "300000"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    assert r.stdout.decode().split()[-1] == "0"
    # the restatement's bin on the cases the reference's own arithmetic decides
    assert ref.reg2bin(-1, 0) == 4680 and ref.reg2bin(0, 1) == 4681 and ref.reg2bin(16383, 16385) == 585 and ref.reg2bin(0, 1 << 29) == 0


@pytest.mark.parametrize("name", ["issue_356.sam", "ex1_header_500.sam"])
def test_golden_lines_round_trip(name):
    """every record line -> record (samin_ref) -> line (sam_ref) is the line again"""
    text, lines = ref.split_sam(open(os.path.join(GOLDEN, name), "rb").read())
    names = [n for n, _ in ref.header_references(text)]
    assert len(lines) > 10
    for l in lines:
        assert sam_ref.sam_line(ref.record(l, names), names) == l + b"\n", l[:100]
