"""`sambamba index -F` on the device -- sbx_index_fasta: K15a's line starts and K17 (fasta.hip) per chunk, the carry of
fasta_core.hpp across chunks -- through the C ABI, the Python API and `sbx-index -F`, against the Python restatement tests/fai_ref.py
and the reference's own expected text.  The output must not depend on where the chunks are cut."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import fai_ref as ref
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

FASTA = os.path.join(GOLDEN, "test.fasta")
CHUNKS = ("16", "48", "4096", None)         # SBX_FASTA_CHUNK_BYTES; None: the default


def cli(args, env=None):
    from sambamba_amd import index_cli_path
    return subprocess.run([index_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def set_chunk(monkeypatch, chunk):
    if chunk is None:
        monkeypatch.delenv("SBX_FASTA_CHUNK_BYTES", raising=False)
    else:
        monkeypatch.setenv("SBX_FASTA_CHUNK_BYTES", chunk)


def index(path, text, out):
    """("ok", .fai bytes, stats) or ("error", code, message); the .fai must not exist after a failure"""
    import sambamba_amd
    with open(path, "wb") as fh:
        fh.write(text)
    if os.path.exists(out):
        os.remove(out)
    try:
        st = sambamba_amd.index_fasta(path, out)
    except sambamba_amd.SbxError as e:
        assert not os.path.exists(out)
        return ("error", e.code, e.msg)
    return ("ok", open(out, "rb").read(), st)


def check(named, tmp_path):
    path, out = str(tmp_path / "in.fa"), str(tmp_path / "out.fai")
    for name, text in named.items():
        want = ref.expected(text)
        got = index(path, text, out)
        if want[0] == "ok":
            assert got[:2] == want, (name, got, want)
            assert got[2]["n_bytes"] == len(text) and got[2]["n_sequences"] == want[1].count(b"\n")
            assert got[2]["n_lines"] == len(ref.lines_of(text, ref.terminator(text)))
        else:
            exc = ref.SequenceBeforeHeader() if want[0] == "seq" else ref.BareNewline(want[1], want[2])
            assert got == ("error", -3, ref.complaint(path, exc)), (name, got, want)


def test_golden_file_through_every_interface(tmp_path):
    import sambamba_amd
    from sambamba_amd._lib import FastaStats
    L = sambamba_amd.lib()
    out = str(tmp_path / "abi.fai")
    st, err = FastaStats(), C.create_string_buffer(512)
    assert L.sbx_index_fasta(FASTA.encode(), out.encode(), -1, C.byref(st), err, 512) == 0, err.value
    assert open(out, "rb").read() == ref.GOLDEN_FAI
    assert (st.n_sequences, st.n_lines, st.n_bytes, st.n_chunks) == (2, 7, 127, 1)
    fa = str(tmp_path / "test.fasta")
    with open(fa, "wb") as fh:
        fh.write(open(FASTA, "rb").read())
    st = sambamba_amd.index_fasta(fa)
    assert open(fa + ".fai", "rb").read() == ref.GOLDEN_FAI and st["n_sequences"] == 2
    os.remove(fa + ".fai")
    r = cli(["-F", fa])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"Indexing FASTA file...\n")
    assert open(fa + ".fai", "rb").read() == ref.GOLDEN_FAI
    named = str(tmp_path / "named.fai")
    r = cli([fa, named, "--fasta-input", "-p"], env={"SBX_FASTA_CHUNK_BYTES": "16", "SBX_TIMING": "1"})
    lines = r.stderr.decode().splitlines()
    assert (r.returncode, r.stdout, lines[:2]) == (0, b"", ["Indexing FASTA file...", "[info] progressbar is unavailable for FASTA input"])
    assert len(lines) == 3 and lines[2].startswith("[sbx] fasta: n_sequences=2 n_lines=7 n_bytes=127 n_chunks=8 chunk_bytes=16 terminator=lf ")
    assert open(named, "rb").read() == ref.GOLDEN_FAI


@pytest.mark.parametrize("chunk", CHUNKS, ids=[c or "default" for c in CHUNKS])
def test_edge_texts(chunk, tmp_path, monkeypatch):
    set_chunk(monkeypatch, chunk)
    named = dict(ref.CASES)
    named["golden"] = open(FASTA, "rb").read()
    check(named, tmp_path)


@pytest.mark.parametrize("chunk", CHUNKS, ids=[c or "default" for c in CHUNKS])
def test_random_texts(chunk, tmp_path, monkeypatch):
    set_chunk(monkeypatch, chunk)
    check({"random %d" % k: t for k, t in enumerate(ref.random_cases())}, tmp_path)


@pytest.mark.parametrize("chunk", CHUNKS, ids=[c or "default" for c in CHUNKS])
def test_refusals(chunk, tmp_path, monkeypatch):
    set_chunk(monkeypatch, chunk)
    check(ref.ERRORS, tmp_path)
    path = str(tmp_path / "in.fa")
    with open(path, "wb") as fh:
        fh.write(ref.ERRORS["bare_newline"])
    r = cli(["-F", path])
    want = ref.complaint(path, ref.BareNewline(4, 2))
    assert (r.returncode, r.stdout, r.stderr) == (1, b"", ("Indexing FASTA file...\nsbx-index: " + want + "\n").encode())
    assert not os.path.exists(path + ".fai")
    assert "4 lines end in '\\n' without '\\r'" in want and want.endswith("the first is line 2")


def big_text(kind, seed=5):
    """about 3 MiB: 40 sequences, wrapped at 60 / unwrapped / wrapped at 60 with "\\r\\n" """
    rng = random.Random(seed)
    term = b"\r\n" if kind == "crlf" else b"\n"
    out = []
    for k in range(40):
        n = rng.randrange(40000, 115000)
        seq = bytes(rng.choice(b"ACGT") for _ in range(997)) * (n // 997 + 1)
        seq = seq[:n]
        out.append(b">seq%d description %d" % (k, n))
        if kind == "unwrapped":
            out.append(seq)
        else:
            out += [seq[i:i + 60] for i in range(0, n, 60)]
    return term.join(out) + term


@pytest.mark.parametrize("kind", ["wrapped", "unwrapped", "crlf"])
def test_three_mebibytes_in_chunks_and_whole(kind, tmp_path, monkeypatch):
    text = big_text(kind)
    assert 2 << 20 < len(text) < 5 << 20
    want = ref.fai(text)
    assert want.count(b"\n") == 40
    path = str(tmp_path / "big.fa")
    monkeypatch.delenv("SBX_FASTA_CHUNK_BYTES", raising=False)
    whole = index(path, text, str(tmp_path / "whole.fai"))
    assert whole[:2] == ("ok", want) and whole[2]["n_chunks"] == 1
    monkeypatch.setenv("SBX_FASTA_CHUNK_BYTES", str(64 << 10))
    cut = index(path, text, str(tmp_path / "cut.fai"))
    assert cut[:2] == ("ok", want) and cut[2]["n_chunks"] == (len(text) + (64 << 10) - 1) // (64 << 10)
    assert cut[2]["n_lines"] == whole[2]["n_lines"] == len(ref.lines_of(text, ref.terminator(text)))


# ---- the scans behind K15a and K17a (launch_scan64) ---------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", ["4096", None], ids=["4096", "default"])
def test_line_counts_around_the_group_of_256(chunk, tmp_path, monkeypatch):
    """255 .. 258 lines: 0, 1 and 2 groups of inner lines (0 and 1 lines are "empty" and "only_header_nl" of the edge texts)"""
    set_chunk(monkeypatch, chunk)
    named = {}
    for n in (2, 255, 256, 257, 258):
        lines = [b">s%d" % k if k % 3 == 0 else b"ACGTACGTAC" for k in range(n)]
        named["%d lines" % n] = b"\n".join(lines) + b"\n"
        named["%d lines, open end" % n] = b"\n".join(lines)
    check(named, tmp_path)


def test_more_tiles_and_groups_than_one_round_of_the_scan(tmp_path, monkeypatch):
    """One chunk of more than 1024 text tiles of 4096 bytes and more than 1024 groups of 256 inner lines: launch_scan64 carries its sum
    from one round of 1024 values into the next, for the tile bases of K15a and for the segment numbers of K17a.  The same file in
    chunks of 1 MiB keeps every scan inside one round."""
    rng = random.Random(11)
    out = []
    for k in range(125000):
        out.append(b">s%d" % k)
        out += [b"ACGTTGCAAC"] * rng.choice((2, 3)) if k % 1000 else [b"ACGTTGCAAC", b"ACG"]
    text = b"\n".join(out) + b"\n"
    n_lines = len(out)
    assert len(text) > 1024 * 4096 + 4096 and n_lines - 1 > 1024 * 256 + 256
    want = ref.fai(text)
    assert want.count(b"\n") == 125000
    path = str(tmp_path / "many.fa")
    monkeypatch.delenv("SBX_FASTA_CHUNK_BYTES", raising=False)
    whole = index(path, text, str(tmp_path / "whole.fai"))
    assert whole[:2] == ("ok", want) and whole[2]["n_chunks"] == 1 and whole[2]["n_lines"] == n_lines
    monkeypatch.setenv("SBX_FASTA_CHUNK_BYTES", str(1 << 20))
    assert (1 << 20) < 1024 * 4096 and max(text[i:i + (1 << 20)].count(b"\n") for i in range(0, len(text), 1 << 20)) < 1024 * 256
    cut = index(path, text, str(tmp_path / "cut.fai"))
    assert cut[:2] == ("ok", want) and cut[2]["n_chunks"] == (len(text) + (1 << 20) - 1) >> 20


def test_output_must_not_be_the_input(tmp_path):
    import sambamba_amd
    path = str(tmp_path / "in.fa")
    with open(path, "wb") as fh:
        fh.write(b">a\nAC\n")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.index_fasta(path, path)
    assert ei.value.code == -1 and open(path, "rb").read() == b">a\nAC\n"
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.index_fasta(str(tmp_path / "missing.fa"))
    assert ei.value.code == -2 and not os.path.exists(str(tmp_path / "missing.fa.fai"))


def test_abi_sizeof_fasta_stats():
    import sambamba_amd
    from sambamba_amd._lib import FastaStats, FixbinsStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_fasta_stats") == C.sizeof(FastaStats) == 3 * 8 + 2 * 4 + 3 * 8
    assert L.sbx_abi_sizeof(b"sbx_fixbins_stats") == C.sizeof(FixbinsStats) == 5 * 8 + 2 * 4 + 6 * 8
