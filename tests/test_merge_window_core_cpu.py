"""The pieces of a rewritten record clipped to a window of the merged stream (sambamba_amd/csrc/mergewin_core.hpp: what K11c writes
when sbx_merge_bam keeps no record store), compiled for the host with g++ under -fsanitize=address,undefined into
tests/native/mergewin_host.cpp and run as a program of its own: for every record shape, destination and window the plan reproduces
the slice of the reference rewrite, writes each byte once and nothing outside the window.  Also here: the layout of
sbx_merge_window_stats and the words of the three refusals of the windowed writer for merge.  No GPU needed."""
import ctypes as C
import os
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "mergewin_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mergewin") / "mergewin_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, args):
    return subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE)


def _records(lo, hi):
    """How many record shapes the program must have tried for old lengths lo .. hi: no patch; one patch of old length o and new
    length 0 .. 5 at each distinct place of (36, middle, end); two patches in each distinct layout of (both behind byte 36, first
    and last, both at the end, apart)."""
    total = 0
    for n in range(lo, hi + 1):
        total += 1
        for o in range(6):
            if 36 + o <= n:
                end = n - o
                total += 6 * len({36, (36 + end) // 2, end})
        for o1 in range(6):
            for o2 in range(6):
                if 36 + o1 + o2 <= n:
                    end2 = n - o2
                    third = (end2 - o1 - 36) // 3
                    total += 36 * len({(36, 36 + o1), (36, end2), (end2 - o1, end2), (36 + third, end2 - third)})
    return total


@pytest.mark.parametrize("lo,hi", [(36, 58), (59, 70), (71, 80)])
def test_every_clip_of_a_rewritten_record(host, lo, hi):
    r = run(host, ["exhaustive", lo, hi])
    assert r.returncode == 0, r.stderr.decode()
    f = r.stdout.decode().split()
    assert f[0::2] == ["records", "plans", "stretches", "max"]
    records, plans, stretches, most = (int(x) for x in f[1::2])
    assert records == _records(lo, hi)
    # 7 destinations, windows of 1, 2 and 3 pieces: at least the windows that cover the shortest record, for every shape
    assert plans >= records * 7 * (-(-36 // 7) + -(-36 // 14) + -(-36 // 21))
    # two patches make six stretches, never more; a window of three pieces holds all six only of a short record
    assert most == (6 if lo == 36 else 5) and stretches > plans


def test_plans_at_named_edges(host):
    """A record of 60 bytes at 100 of the stream whose id at [40, 43) becomes 5 bytes and whose id at [50, 52) becomes 1 byte: 61
    bytes, [100, 161).  Lines: kind (0 fixed, 1 source, 2 blob), source offset, window offset, length.  The blob offsets of the
    program are 1000 and 2000."""
    def plan(w0, w1, patches=(40, 3, 5, 50, 2, 1)):
        r = run(host, ["one", 60, 100, w0, w1] + list(patches))
        assert r.returncode == 0, r.stderr
        return [tuple(int(x) for x in ln.split()) for ln in r.stdout.decode().splitlines()]
    whole = [(0, 0, 0, 36), (1, 36, 36, 4), (2, 1000, 40, 5), (1, 43, 45, 7), (2, 2000, 52, 1), (1, 52, 53, 8)]
    assert plan(100, 161) == whole
    assert plan(0, 100) == [] and plan(161, 300) == []
    assert plan(101, 161)[0] == (0, 1, 0, 35)                   # one byte into block_size
    assert plan(0, 106) == [(0, 0, 100, 6)]                     # the window ends inside ref_id
    assert plan(126, 128) == [(0, 26, 0, 2)]                    # ... lies inside next_ref_id
    assert plan(140, 141) == [(2, 1000, 0, 1)]                  # the first byte of a new id
    assert plan(144, 145) == [(2, 1004, 0, 1)]                  # its last byte
    assert plan(100, 145) == whole[:3] and plan(145, 161) == [(1, 43, 0, 7), (2, 2000, 7, 1), (1, 52, 8, 8)]     # between an id and the stretch behind it
    assert plan(152, 153) == [(2, 2000, 0, 1)]
    # no patch and nothing renumbered: the fixed part and one stretch
    assert plan(100, 160, ()) == [(0, 0, 0, 36), (1, 36, 36, 24)]
    assert plan(136, 160, ()) == [(1, 36, 0, 24)]
    # ids of no bytes on either side leave no stretch behind
    assert plan(100, 200, (36, 0, 0, 60, 0, 0)) == [(0, 0, 0, 36), (1, 36, 36, 24)]
    assert plan(100, 200, (36, 4, 0, 40, 20, 0)) == [(0, 0, 0, 36)]


def test_refusals_in_the_words_of_merge(host):
    r = run(host, ["words"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().splitlines() == [
        "the input changed while it was being merged (a batch of the read pass holds other records than before)",
        "the input changed while it was being merged (bytes [65280, 130560) of the merged stream: 65279 record bytes arrived where 65280 belong, "
        "2 record(s) are not the ones the key pass read)",
        "the files do not fit the device: merging them in windows needs 1000 bytes of device memory (a window of one piece and the encoder, "
        "next to the read batch and 12 bytes per record), 10 are free"]
    text = open(os.path.join(ROOT, "sambamba_amd", "csrc", "sort_core.hpp")).read()
    assert "kMergeWindowWords" in text and all(w in text for w in ('"merging them"', '"it was being merged"', '"merged stream"'))


def test_window_stats_of_the_abi():
    import sambamba_amd
    from sambamba_amd._lib import MergeStats, MergeWindowStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_merge_window_stats") == C.sizeof(MergeWindowStats) == 5 * 4 + 4 + 8 + 4 * 8
    assert [k for k, _ in MergeWindowStats._fields_] == ["struct_size", "n_windows", "n_batch_runs", "n_batches_skipped", "n_input_opens",
                                                         "window_bytes", "ms_dest", "ms_scatter", "ms_inflate_replay", "ms_index_replay"]
    assert MergeWindowStats.struct_size.offset == 0 and MergeWindowStats.window_bytes.offset == 24
    # sbx_merge_stats keeps its layout
    assert L.sbx_abi_sizeof(b"sbx_merge_stats") == C.sizeof(MergeStats) == 7 * 8 + 4 * 4 + 7 * 8
    assert hasattr(L, "sbx_merge_bam_run") and hasattr(L, "sbx_merge_bam")
    header = open(os.path.join(ROOT, "include", "sbx_depth.h")).read()
    assert "uint32_t n_windows, n_batch_runs, n_batches_skipped, n_input_opens;" in header and "} sbx_merge_window_stats;" in header
    d = open(os.path.join(ROOT, "d", "sbx_depth.d")).read()
    assert "uint struct_size; uint n_windows; uint n_batch_runs; uint n_batches_skipped; uint n_input_opens;" in d and "sbx_merge_bam_run" in d
