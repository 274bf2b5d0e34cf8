"""K1b's dependency rounds and the one-round fast path on the CPU.  `lz::frontier_blocked` (sambamba_amd/csrc/lz77_copy.hpp) is the
`__host__ __device__` predicate `lz77_resolve_body` evaluates with kFast; tests/cpp/lz77_rounds_host.cpp runs it inside the lock-step
model of the rounds, batch by batch, on the hand-assembled blocks of tests/lz77_round_cases.py, against zlib's inflate of the same
streams: a batch for which no lane is blocked must resolve in ONE round, without ranges, searches or masks, to zlib's bytes (and the
exact rule must find nothing to wait for in it); a batch in which lane k's source is lane k - 1's destination must not take the fast
path and needs as many rounds as its chain is deep.  The harness is also built with -fsanitize=address,undefined and run as it is.
The same blocks run on the device in tests/test_gpu_inflate_rounds.py."""
import os
import struct
import subprocess
import zlib

import pytest

from tests.lz77_round_cases import batches_of, cases
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "lz77_rounds_host.cpp")


@pytest.fixture(scope="module")
def table():
    return cases()


@pytest.fixture(scope="module")
def case_file(tmp_path_factory, table):
    path = str(tmp_path_factory.mktemp("lz77_rounds") / "cases.bin")
    with open(path, "wb") as fh:
        for name, stream, payload, entries, literals, _, _ in table:
            assert zlib.decompress(stream, -15) == payload
            fh.write(struct.pack("<I", len(name)) + name.encode())
            fh.write(struct.pack("<I", len(stream)) + stream)
            fh.write(struct.pack("<I%dI" % len(entries), len(entries), *entries))
            fh.write(struct.pack("<I", len(literals)) + literals)
    return path


def _build(tmp_path_factory, flags):
    exe = str(tmp_path_factory.mktemp("lz77_rounds_exe") / "lz77_rounds_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror"] + flags + ["-o", exe, SRC, "-lz"])
    return exe


def _run(exe, case_file):
    p = subprocess.run([exe, case_file], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert p.returncode == 0, p.stdout + p.stderr
    rows = {}
    for line in p.stdout.splitlines():
        name, letters, rounds, takes = line.split()
        rows[name] = (letters, [int(x) for x in rounds.split(",")], [int(x) for x in takes.split(",")])
    return rows


@pytest.fixture(scope="module")
def rows(tmp_path_factory, case_file):
    return _run(_build(tmp_path_factory, []), case_file)


def test_every_block_resolves_to_zlibs_bytes(rows, table):
    """Exit status 0: every batch of every block equals zlib right after its rounds, fast batches after exactly one."""
    assert set(rows) == {c[0] for c in table}
    for name, _, _, entries, _, _, _ in table:
        letters, rounds, takes = rows[name]
        assert takes == [n for n, _ in batches_of(entries)], name
        assert len(letters) == len(rounds) == len(takes)
        for letter, r in zip(letters, rounds):
            assert (letter == "n") == (r == 0) and (letter != "f" or r == 1), (name, letters, rounds)


def test_predicate_and_rounds_of_the_hand_built_batches(rows, table):
    for name, _, _, _, _, letters, rounds in table:
        if letters is not None:
            assert rows[name][0] == letters, name
        if rounds is not None:
            assert rows[name][1] == rounds, name


def test_predicate_is_false_where_a_source_is_the_destination_in_front(rows):
    """c_chain_*: lane k copies what lane k - 1 writes.  Not one round, not the fast path."""
    for depth in (2, 3, 63):
        letters, rounds, takes = rows["c_chain_%d" % depth]
        assert letters == "x" and rounds == [depth] and takes == [64]


def test_random_stream_takes_both_paths_and_slides(rows, table):
    letters, rounds, _ = rows["random_tokens"]
    payload = [c[2] for c in table if c[0] == "random_tokens"][0]
    assert len(payload) > 2048 + 1024 + 1536 and "x" in letters and max(rounds) > 2


def test_span_cut_batches(rows):
    assert rows["e_span_cuts"][2] == [2, 63, 2, 1]


def test_harness_under_address_and_undefined_sanitizers(tmp_path_factory, case_file, rows):
    san = _run(_build(tmp_path_factory, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), case_file)
    assert san == rows
