"""K1b's write-out on the CPU: `lz::plan_writeout` and `lz::writeout_lane` (sambamba_amd/csrc/lz77_copy.hpp) are `__host__ __device__`
-- phase C of `lz77_resolve_body` calls them; the harness tests/cpp/lz77_writeout_host.cpp runs them batch by batch, lane by lane, next
to a model of the wave's window and its slide.  For every alignment 0 .. 15 of a block's first byte, batches of 1, 15, 16, 17, 1023,
1024, 1025 and kSpanMax bytes (alone, first, last, repeated until the window has slid several times) and random batch sizes adding up
to blocks of 0, 1, 15, 16, 17, 33, 65280 and 65535 bytes, it checks that the stores cover the block exactly, each byte once and
nothing around it; that every 16-byte store is aligned in absolute address; that fewer than 16 bytes are carried between batches; and
that the slide only drops bytes that are in HBM.  The same statements run on the GPU (tests/test_gpu_inflate_writeout.py)."""
import os
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "lz77_writeout_host.cpp")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lz77_writeout") / "lz77_writeout_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, SRC])
    return exe


def test_writeout_plan_every_alignment_and_batch_size(harness):
    p = subprocess.run([harness], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stderr
    blocks, batches, bad = (int(x) for x in p.stdout.split())
    assert bad == 0
    # 16 alignments x (8 sizes x (2 + 8 x 2) + 6 x 24 + 2 x 6 random blocks)
    assert blocks == 16 * (8 * 18 + 6 * 24 + 2 * 6) and batches > 10 * blocks


def test_kernel_calls_the_plan():
    """Phase C of the product body is the plan and the lane function of lz77_copy.hpp, nothing of its own."""
    src = open(os.path.join(ROOT, "sambamba_amd", "csrc", "inflate.hip")).read()
    body = src[src.index("void lz77_resolve_body("):src.index("#define SBX_LZ77_ARGS")]
    assert "lz::plan_writeout(" in body and "lz::writeout_lane(" in body
