"""The window arithmetic of the windowed sort (sambamba_amd/csrc/sort_core.hpp: plan_windows, span_meets_window, the clip of a record
to a window, window_refusal), compiled for the host with g++ under -fsanitize=address,undefined into tests/native/sortwin_host.cpp and
run as a program of its own: the windows cover the stream exactly, in whole pieces, none empty; every byte of every window is written
exactly once by the batches the span test admits; the two consistency checks word their refusal -- and the `n_windows` word of
sbx_sort_stats sits where `reserved` sat.  No GPU needed."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "sortwin_host.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sortwin") / "sortwin_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC])
    return exe


def run(exe, args, data=b""):
    return subprocess.run([exe] + [str(a) for a in args], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE)


@pytest.mark.parametrize("piece", [1, 7, 0xFF00, 32768 * 0xFF00])
def test_window_plan_is_exact(host, piece):
    """Totals of 0 .. 40 pieces +- 1 byte, windows of 1 .. 5 pieces (given exactly, one byte short and one byte above the size
    below: all round UP): exact cover, every edge but the last a piece multiple, no empty window."""
    r = run(host, ["plan", piece, 40, 5])
    assert r.returncode == 0, r.stderr
    lines = r.stdout.decode().splitlines()
    seen = set()
    for ln in lines:
        head, _, tail = ln.partition(":")
        total, wb = (int(x) for x in head.split())
        xs = [int(x) for x in tail.split()]
        wins = list(zip(xs[0::2], xs[1::2]))
        span = max(1, -(-wb // piece)) * piece
        assert 1 <= span // piece <= 5 and span >= wb > span - piece
        seen.add((total, span // piece))
        assert len(wins) == -(-total // span), ln                  # no window more than needed: none is empty, also for an exact multiple
        at = 0
        for w0, w1 in wins:
            assert w0 == at and w1 > w0 and w0 % piece == 0 and w1 - w0 <= span, ln
            at = w1
        assert at == total, ln                                     # the last window ends at total
        assert all(w1 - w0 == span for w0, w1 in wins[:-1]), ln    # whole pieces: only the last window may be shorter
    totals = {k * piece + d for k in range(41) for d in (-1, 0, 1) if k * piece + d >= 0}
    assert seen == {(t, w) for t in totals for w in range(1, 6)}


def _clip_case(host, hlen, piece, window, batch, lens, order):
    """order[q] = the record at place q of the sorted stream."""
    n = len(lens)
    rank = [0] * n
    for q, i in enumerate(order):
        rank[i] = q
    r = run(host, ["clip", hlen, piece, window, batch], "".join("%d %d\n" % (lens[i], rank[i]) for i in range(n)).encode())
    assert r.returncode == 0, r.stderr
    # the byte-by-byte model: the stream is the header and then the records in sorted order
    want = bytes(0x80 | (j % 127) for j in range(hlen)) + b"".join(bytes((i * 131 + j * 7 + 3) % 127 for j in range(lens[i])) for i in order)
    assert r.stdout == want
    wins = [[int(x) for x in ln.split()[1:]] for ln in r.stderr.decode().splitlines() if ln.startswith("window ")]
    span = max(1, -(-window // piece)) * piece
    assert len(wins) == -(-len(want) // span)
    for k, (kk, w0, w1, unwritten, twice, outside, runs, skipped, whole) in enumerate(wins):
        assert (kk, w0, w1) == (k, k * span, min(len(want), (k + 1) * span))
        assert (unwritten, twice, outside, whole) == (0, 0, 0, 1), (k, wins[k])
        assert runs + skipped == -(-n // batch)
    return wins


@pytest.mark.parametrize("piece,window", [(64, 64), (64, 128), (64, 100), (50, 150)])
def test_clip_to_windows_writes_every_byte_once(host, piece, window):
    rng = random.Random(piece * 1000 + window)
    span = -(-window // piece) * piece
    cases = []
    for seed in range(3):
        lens = [rng.randrange(36, 201) for _ in range(rng.randrange(1, 90))]
        order = list(range(len(lens)))
        rng.shuffle(order)
        cases.append((rng.randrange(0, 3 * span), lens, order))
    # window edges one byte into a record, one byte before a record's end, exactly between two records
    cases.append((span + 1, [piece] * 13, list(range(13))))
    cases.append((span - 1, [piece] * 13, list(range(13))))
    cases.append((span, [piece] * 13, list(reversed(range(13)))))
    # a record that spans a whole window (three windows write a part of it), minimal records next to it
    cases.append((17, [36, 2 * span + 100, 36, 3 * span, 36], [4, 1, 0, 3, 2]))
    # the header longer than two windows, ending at a window edge; no records; a total that is a multiple of the window
    cases.append((2 * span + 37, [40, 50, 60], [2, 0, 1]))
    cases.append((2 * span, [40, 50, 60], [0, 1, 2]))
    cases.append((2 * span + 5, [], []))
    cases.append((span, [], []))
    lens = [rng.randrange(36, 201) for _ in range(20)]
    lens.append(5 * span - (29 + sum(lens)) % span)
    assert (29 + sum(lens)) % span == 0
    cases.append((29, lens, list(range(len(lens)))))
    for hlen, lens, order in cases:
        for batch in (1, 7, 1000):
            _clip_case(host, hlen, piece, window, batch, lens, order)


def test_batches_in_order_meet_few_windows(host):
    """Records already in order: a batch is run only by the windows its span touches; shuffled, every window may need every batch."""
    rng = random.Random(4)
    lens = [rng.randrange(36, 201) for _ in range(600)]
    n_batches = 600 // 25
    wins = _clip_case(host, 100, 64, 64 * 40, 25, lens, list(range(600)))
    assert len(wins) >= 6 and sum(w[6] for w in wins) <= n_batches + 2 * len(wins) and sum(w[7] for w in wins) > 0
    order = list(range(600))
    rng.shuffle(order)
    wins = _clip_case(host, 100, 64, 64 * 40, 25, lens, order)
    assert sum(w[6] for w in wins) > n_batches + 2 * len(wins)


def test_window_refusal_wording(host):
    # window [100, 300) of a stream whose header is 150 bytes long: 150 record bytes belong there
    assert run(host, ["refusal", 100, 300, 150, 150, 0]).returncode == 0
    assert run(host, ["refusal", 0, 100, 150, 0, 0]).returncode == 0           # a window of header bytes only
    assert run(host, ["refusal", 300, 500, 150, 200, 0]).returncode == 0       # a window behind the header
    for args in ([100, 300, 150, 149, 0], [100, 300, 150, 151, 0], [100, 300, 150, 150, 1], [0, 100, 150, 1, 0]):
        r = run(host, ["refusal"] + args)
        assert r.returncode == 3 and b"the input changed while it was being sorted" in r.stdout, args
    # the whole sentence, in the words of either command: the windowed writer is one, the phrases are the command's
    phrases = {"sort": ("it was being sorted", "sorted stream", "the keys were taken from"),
               "markdup": ("its duplicates were being marked", "output stream", "the key pass read")}
    for cmd, (doing, stream, source) in phrases.items():
        # (window, header bytes, record bytes arrived, mismatches) -> record bytes that belong: a record that is another one; a byte
        # short in the window that holds the 100 header bytes; both at once
        for args, belong in (([65280, 130560, 100, 65280, 2], 65280), ([0, 65280, 100, 65179, 0], 65180), ([65280, 130560, 100, 65279, 2], 65280)):
            r = run(host, ["refusal"] + args + [cmd])
            want = ("the input changed while %s (bytes [%d, %d) of the %s: %d record bytes arrived where %d belong, %d record(s) are not the ones %s)"
                    % (doing, args[0], args[1], stream, args[3], belong, args[4], source))
            assert (r.returncode, r.stdout.decode()) == (3, want)
        assert run(host, ["refusal", 65280, 130560, 100, 65280, 0, cmd]).returncode == 0
    assert run(host, ["refusal", 65280, 130560, 100, 65279, 2, "markdup"]).stdout == (
        b"the input changed while its duplicates were being marked (bytes [65280, 130560) of the output stream: 65279 record bytes arrived "
        b"where 65280 belong, 2 record(s) are not the ones the key pass read)")
    assert run(host, ["refusal", 0, 1, 0, 0, 0, "view"]).returncode == 2
    # the refusal of a batch that came out differently, and of a file for which not even one window fits
    assert run(host, ["words", "sort"]).stdout.decode().splitlines() == [
        "the input changed while it was being sorted (a batch of the read pass holds other records than before)",
        "the file does not fit the device: sorting it in windows needs 1000 bytes of device memory (one window of one piece and the encoder, "
        "next to the read batch and 12 bytes per record), 10 are free"]
    assert run(host, ["words", "markdup"]).stdout.decode().splitlines() == [
        "the input changed while its duplicates were being marked (a batch of the read pass holds other records than before)",
        "the file does not fit the device: marking its duplicates in windows needs 1000 bytes of device memory (a window of one piece and the "
        "encoder, next to the read batch and 17 bytes per record), 10 are free"]


def test_n_windows_word_of_the_stats():
    import sambamba_amd
    from sambamba_amd._lib import SortStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_sort_stats") == C.sizeof(SortStats) == 112
    names = [k for k, _ in SortStats._fields_]
    assert "n_windows" in names and "reserved" not in names
    # where `reserved` was: the fourth 32-bit word behind the five 64-bit counters, in front of the milliseconds
    assert SortStats.n_windows.offset == 5 * 8 + 3 * 4 == SortStats.ms_inflate.offset - 4
    assert names[names.index("n_windows") - 1] == "n_batches"
    header = open(os.path.join(ROOT, "include", "sbx_depth.h")).read()
    assert "key_bits, n_sort_passes, n_batches, n_windows;" in header
    assert "uint key_bits; uint n_sort_passes; uint n_batches; uint n_windows;" in open(os.path.join(ROOT, "d", "sbx_depth.d")).read()
