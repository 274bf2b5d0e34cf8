"""The streamed path of `fixbins` (sbx_fixbins_run): no record store; per batch K16b computes the bins from the records where K1 left
them and K21 (stream.hip) writes the two bytes while it copies the records into the staging window of engine_streamout.hpp.

Every case writes the output once on the resident path (SBX_STREAM_WINDOW_BYTES unset) and once streamed with a window of one
65280-byte piece, and asserts that the two files are identical, that n_bins_changed agrees and that the streamed stats report the
expected number of windows.  On a library without the feature the hook is ignored and no stream stats exist."""
import filecmp
import os
import random
import struct

import pytest

from tests import bamgen
from tests import bins_cases as bc
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream
from tests.test_gpu_fixbins import check_file, fixed_stream

pytestmark = pytest.mark.gpu

PIECE = 0xFF00
COPIES = 7          # the ~430 records of bins_cases, this many times over: three windows


def both(monkeypatch, path, tmp_path, tag="o", batch=bc.BATCH):
    import sambamba_amd
    monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES", raising=False)
    a, b = str(tmp_path / (tag + ".resident.bam")), str(tmp_path / (tag + ".streamed.bam"))
    st_r = sambamba_amd.fixbins(path, a)
    monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", "1")
    st_s = sambamba_amd.fixbins(path, b)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES")
    print("%s: stream_bytes %d n_batches %d n_windows %d n_pack_launches %d ms_pack %.3f" % (
        tag, st_s["stream_bytes"], st_s["n_batches"], st_s["n_windows"], st_s["n_pack_launches"], st_s["ms_pack"]))
    assert filecmp.cmp(a, b, shallow=False)
    assert (st_r["n_windows"], st_r["window_bytes"], st_r["n_pack_launches"], st_r["ms_pack"]) == (0, 0, 0, 0.0)
    assert st_s["n_windows"] == max(1, -(-st_s["stream_bytes"] // PIECE)) and st_s["window_bytes"] == PIECE
    for k in ("n_records", "n_bins_changed", "inflated_bytes", "stream_bytes", "compressed_bytes", "n_batches"):
        assert st_r[k] == st_s[k], k
    assert st_s["compressed_bytes"] == os.path.getsize(b)
    return st_r, st_s


def header_text(pad):
    return ("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bc.REFS) + "@CO\t" + "x" * pad + "\n")


def spoiled_records(seed):
    recs, _ = bc.records()
    recs = recs * COPIES
    rng = random.Random(seed)
    return bc.with_bins(recs, {i: rng.randrange(0, 1 << 16) for i in range(len(recs))})


@pytest.mark.parametrize("byte_at_window_end", [14, 15])
def test_wrong_bins_and_a_bin_field_at_a_window_edge(tmp_path, monkeypatch, byte_at_window_end):
    """every bin wrong; the header is padded so that byte 14 (then: byte 15) of one record is the last byte of the first window --
    with 14 the two bytes of its bin go to different windows -- and the same for another record at the end of the second window
    as far as the lengths allow"""
    recs = spoiled_records(11 + byte_at_window_end)
    info = bc.write(tmp_path / "probe.bam", recs, text=header_text(100))
    # the first record that starts in the last 600 bytes of window 0
    k = next(i for i, r in enumerate(info["records"]) if PIECE - 600 <= r[3] < PIECE - 300)
    pad = 100 + (PIECE - 1) - (info["records"][k][3] + byte_at_window_end)
    path = str(tmp_path / "edge.bam")
    info = bc.write(path, recs, text=header_text(pad))
    assert info["records"][k][3] + byte_at_window_end == PIECE - 1                   # (checked on the CPU)
    stream = inflate(path)
    want, changed = fixed_stream(stream)
    assert struct.unpack_from("<H", recs[k], 14)[0] != bc.expected_bin(recs[k]) and changed > len(recs) - 5 * COPIES
    st_r, st_s = both(monkeypatch, path, tmp_path)
    check_file(str(tmp_path / "o.resident.bam"), want)
    assert st_s["n_bins_changed"] == changed and st_s["n_records"] == len(recs)
    assert st_s["n_windows"] >= 3 and st_s["n_batches"] >= 8
    # the whole file as one batch: several windows inside it
    both(monkeypatch, path, tmp_path, tag="big", batch="100000000")


def test_nothing_to_fix(tmp_path, monkeypatch):
    recs, _ = bc.records()
    path = str(tmp_path / "right.bam")
    bc.write(path, recs * COPIES)
    stream = inflate(path)
    assert fixed_stream(stream) == (stream, 0)
    st_r, st_s = both(monkeypatch, path, tmp_path)
    check_file(str(tmp_path / "o.streamed.bam"), stream)
    assert st_s["n_bins_changed"] == 0 and st_s["n_windows"] >= 3


def test_empty_and_malformed(tmp_path, monkeypatch):
    import sambamba_amd
    path = str(tmp_path / "empty.bam")
    bc.write(path, [])
    _, st = both(monkeypatch, path, tmp_path, tag="empty")
    assert (st["n_records"], st["n_windows"], st["n_pack_launches"]) == (0, 1, 0)
    # a CIGAR count that runs past the record's block_size, in a later batch: SBX_EFORMAT on both paths, and no output file
    recs = spoiled_records(3)
    broken = bytearray(recs[2500])
    struct.pack_into("<H", broken, 16, 4000)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bc.REFS)
    stream = bamgen.bam_header(text, bc.REFS) + b"".join(recs[:2500]) + bytes(broken) + b"".join(recs[2501:])
    bad = str(tmp_path / "bad.bam")
    with open(bad, "wb") as fh:
        fh.write(b"".join(bamgen.bgzf_block(stream[o:o + bc.BLOCK]) for o in range(0, len(stream), bc.BLOCK)) + bamgen.EOF_BLOCK)
    monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", bc.BATCH)
    seen = []
    for hook in (None, "1"):
        if hook:
            monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", hook)
        out = str(tmp_path / "bad.out.bam")
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.fixbins(bad, out)
        seen.append((ei.value.code, ei.value.msg))
        assert not os.path.exists(out)
    assert seen[0] == seen[1] and seen[0][0] == -3


def test_cli_timing_line(tmp_path):
    import subprocess
    from sambamba_amd import fixbins_cli_path
    path = str(tmp_path / "in.bam")
    bc.write(path, spoiled_records(5))
    env = dict(os.environ, SBX_TIMING="1", SBX_BGZF_PIECE_BLOCKS="1", SBX_STREAM_WINDOW_BYTES="1", SBX_INDEX_BATCH_BYTES=bc.BATCH)
    out = str(tmp_path / "cli.bam")
    r = subprocess.run([fixbins_cli_path(), path, out], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.decode().splitlines() if l.startswith("[sbx] stream:")]
    assert len(lines) == 1 and int(lines[0].split("n_windows=")[1].split()[0]) >= 3
    check_file(out, fixed_stream(inflate(path))[0])
