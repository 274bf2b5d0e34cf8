"""K1a's lane program on the CPU over the case table (tests/k1_cases.py): hand-built DEFLATE streams at the decoders' own limits.
tests/cpp/inflate2_host.cpp runs every case through sambamba_amd/csrc/inflate2_core.hpp one lane at a time: a valid stream is decoded
exactly (compared with the payload zlib confirmed when the table was built) or handed to the general kernel, whichever the table says,
with the plain or the general form of the symbol loop as the table says; an invalid one is never accepted.  The harness is built twice:
plainly, and -- it is a stand-alone program -- with AddressSanitizer and UBSan, where every stream has exactly the 128 KiB + 64 readable
bytes behind it that the lane program documents for its prefetch.  The GPU test (tests/test_gpu_k1_edges.py) sends the same table."""
import os
import subprocess
import zlib

import pytest

from tests import k1_cases
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "inflate2_host.cpp")


@pytest.fixture(scope="module")
def case_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("k1") / "cases.bin")
    k1_cases.case_file(k1_cases.CASES, path)
    return path


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("k1_" + request.param) / "inflate2_host")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + flags + ["-o", exe, SRC, "-lz"])
    return exe


def test_table_is_what_zlib_says():
    """Every case against zlib once more, outside the module that built it; nothing is excluded; every limit has its case."""
    names = [c[0] for c in k1_cases.CASES]
    assert len(set(names)) == len(names) and len(k1_cases.VALID) + len(k1_cases.INVALID) == len(names)
    for name, stream, payload, e in k1_cases.CASES:
        if payload is None:
            assert e.path == "reject"
            with pytest.raises((zlib.error, ValueError)):
                k1_cases.reference(stream, e.isize)
        else:
            assert e.path in ("fast", "general") and len(payload) == e.isize <= 65536
            assert zlib.decompress(stream, -15) == payload and k1_cases.reference(stream, e.isize) == payload, name
    for name in ("lit_complete_only_at_15_bits", "dist_complete_at_exactly_13_bits", "max_bit_rate_63_bits_per_iteration"):
        assert k1_cases.BY_NAME[name][3].loops >= 1
    for name in ("lit_complete_at_exactly_14_bits", "nlit_263", "lits_65536_no_match_isize_65536", "most_entries_3_byte_matches_throughout"):
        assert k1_cases.BY_NAME[name][3][:2] == ("fast", 0)
    assert k1_cases.BY_NAME["deflate_blocks_6"][3].path == "fast" and k1_cases.BY_NAME["deflate_blocks_7"][3].path == "general"
    assert all(n in k1_cases.BY_NAME for n in k1_cases.PLACEMENT)


@pytest.mark.parametrize("lane", [0, 17, 63])
def test_lane_program_over_the_table(harness, case_file, lane):
    # (the time limit: a lane program that loops forever fails here; the sanitized run takes about a second)
    p = subprocess.run([harness, "--cases", case_file, str(lane)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    cases, fast, general, rejected, bad = (int(x) for x in p.stdout.split())
    assert bad == 0 and cases == len(k1_cases.CASES)
    assert fast == sum(1 for c in k1_cases.VALID if c[3].path == "fast")
    assert general == sum(1 for c in k1_cases.VALID if c[3].path == "general")
    assert rejected == len(k1_cases.INVALID)
