"""The arithmetic of K21 and of the streamed writer (sambamba_amd/csrc/stream_core.hpp: plan_record, window_record_bytes), compiled
for the host with g++ under -fsanitize=address,undefined into tests/native/stream_host.cpp and run as a program of its own: whatever
the place of a record relative to the staging window, with or without the bin patch, every byte of the window that belongs to the
record is written exactly once with the right value, no byte outside it is touched, and the count K21 reports is their number.
No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "stream_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("stream") / "stream_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, args):
    return subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("window", [1, 15, 16, 17, 65280])
def test_record_against_window(host, window):
    """before, cut at the front, inside, cut at the back, spanning the window, behind it, and every start within 20 bytes of either
    edge; no patch and three bin values; the two bin bytes in different windows."""
    r = run(host, ["plan", window])
    assert r.returncode == 0, r.stderr.decode()
    words = r.stdout.decode().split()
    assert words[0] == "cases" and int(words[1]) > 4000
    # cases in which exactly one of the two bin bytes lies in the window: byte 14 its last byte, or byte 15 its first
    assert words[2] == "patched_split" and int(words[3]) >= 6


@pytest.mark.parametrize("window,hlen", [(64, 100), (64, 128), (50, 7), (65280, 65280 + 17)])
def test_stream_through_windows(host, window, hlen):
    """A header and ten records -- three of them longer than a window, every second one patched -- through consecutive windows: the
    bytes are those of the stream written in one piece, and every window's count is window_record_bytes."""
    r = run(host, ["stream", window, hlen])
    assert r.returncode == 0, r.stderr.decode()
    lens = [36, 40, 200, 3 * window + 36, 36, 77, window, 36, 2 * window + 1, 50]
    want = bytearray(0x80 | (j % 127) for j in range(hlen))
    for i, n in enumerate(lens):
        rec = bytearray((i * 131 + j * 7 + 3) % 127 for j in range(n))
        if i % 2:
            rec[14:16] = (0x1234 + i).to_bytes(2, "little")
        want += rec
    assert r.stdout == bytes(want)
    assert r.stderr.decode().split() == ["windows", str(-(-len(want) // window))]


def test_usage(host):
    assert run(host, []).returncode == 2


def test_stream_stats_layout():
    import sambamba_amd
    from sambamba_amd._lib import EXPORTS, StreamStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_stream_stats") == C.sizeof(StreamStats) == 2 * 8 + 2 * 4 + 8
    assert {"sbx_view_run_streamed", "sbx_fixbins_run"} <= set(EXPORTS)
    assert hasattr(L, "sbx_view_run_streamed") and hasattr(L, "sbx_fixbins_run")
    header = open(os.path.join(ROOT, "include", "sbx_depth.h")).read()
    assert "} sbx_stream_stats;" in header and "sbx_view_run_streamed(" in header and "sbx_fixbins_run(" in header
    d = open(os.path.join(ROOT, "d", "sbx_depth.d")).read()
    assert "struct sbx_stream_stats" in d and "sbx_view_run_streamed(" in d and "sbx_fixbins_run(" in d
