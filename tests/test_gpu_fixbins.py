"""`sambamba fixbins` on the device -- sbx_fixbins: K16b (bins.hip) over the resident record store between the read pass and the BGZF
encoder -- through the Python API and `sbx-fixbins`: the inflated output is the input stream with the bin of every record set by
the Python statement of reg2bin(pos, pos + basesCovered()), and nothing else changed."""
import ctypes as C
import os
import random
import struct
import subprocess

import pytest

from tests import bamgen
from tests import bins_cases as bc
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream
from tests.util import GOLDEN, scan_bgzf

pytestmark = pytest.mark.gpu

FIXTURES = ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates")


def cli(args, env=None):
    from sambamba_amd import fixbins_cli_path
    return subprocess.run([fixbins_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def fixed_stream(stream):
    """(the stream with every bin set right, the number of records whose bin changes)"""
    recs = split_stream(stream)[3]
    head = stream[:len(stream) - sum(len(r) for r in recs)]
    out, changed = [], 0
    for r in recs:
        want = bc.expected_bin(r)
        changed += want != struct.unpack_from("<H", r, 14)[0]
        out.append(r[:14] + struct.pack("<H", want) + r[16:])
    return head + b"".join(out), changed


def check_file(path, want):
    raw = open(path, "rb").read()
    assert raw[-28:] == bamgen.EOF_BLOCK
    _, _, _, isize, _, _ = scan_bgzf(path)
    assert all(int(x) <= 0xFF00 for x in isize) and int(isize[-1]) == 0 and all(int(x) > 0 for x in isize[:-1])
    got = inflate(path)
    assert len(got) == len(want) and got == want


@pytest.fixture(scope="module")
def spoiled(tmp_path_factory):
    """the generated file with every bin replaced by a seeded random 16-bit value: (path, inflated stream, expected stream, changed)"""
    d = tmp_path_factory.mktemp("fixbins")
    recs, _ = bc.records()
    rng = random.Random(11)
    path = str(d / "spoiled.bam")
    bc.write(path, bc.with_bins(recs, {i: rng.randrange(0, 1 << 16) for i in range(len(recs))}))
    stream = inflate(path)
    want, changed = fixed_stream(stream)
    assert changed > len(recs) - 5
    return path, stream, want, changed


def test_every_bin_is_set(spoiled, tmp_path):
    import sambamba_amd
    path, stream, want, changed = spoiled
    out = str(tmp_path / "fixed.bam")
    st = sambamba_amd.fixbins(path, out)
    check_file(out, want)
    n = len(split_stream(stream)[3])
    assert (st["n_records"], st["n_bins_changed"]) == (n, changed)
    assert st["stream_bytes"] == len(want) == st["inflated_bytes"] and st["compressed_bytes"] == os.path.getsize(out)
    # header text and reference list are the input's, byte for byte
    text, refs = split_stream(stream)[:2]
    assert split_stream(inflate(out))[:2] == (text, refs) and b"@PG" not in text
    sambamba_amd.build_index(out, check_bins=True)
    with pytest.raises(sambamba_amd.SbxError):
        sambamba_amd.build_index(path, str(tmp_path / "no.bai"), check_bins=True)
    out_cli = str(tmp_path / "cli.bam")
    r = cli(["-t", "3", "-p", path, out_cli])
    assert (r.returncode, r.stdout, r.stderr) == (0, b"", b"")
    check_file(out_cli, want)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_are_unchanged(name, tmp_path):
    import sambamba_amd
    src = os.path.join(GOLDEN, name + ".bam")
    out = str(tmp_path / "o.bam")
    st = sambamba_amd.fixbins(src, out)
    stream = inflate(src)
    assert fixed_stream(stream) == (stream, 0)
    check_file(out, stream)
    assert st["n_bins_changed"] == 0 and st["n_records"] == len(split_stream(stream)[3])


def test_pieces_and_batches_give_the_same_bytes(spoiled, tmp_path, monkeypatch):
    import sambamba_amd
    path, _, want, changed = spoiled
    out = str(tmp_path / "p.bam")
    r = cli([path, out], env={"SBX_BGZF_PIECE_BLOCKS": "1", "SBX_INDEX_BATCH_BYTES": bc.BATCH, "SBX_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("[sbx] fixbins:")]
    assert len(line) == 1 and "n_bins_changed=%d " % changed in line[0]
    assert int(line[0].split("n_batches=")[1].split()[0]) >= 3
    check_file(out, want)
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", bc.BATCH)
    st = sambamba_amd.fixbins(path, str(tmp_path / "b.bam"))
    assert st["n_batches"] >= 3 and st["n_bins_changed"] == changed
    check_file(str(tmp_path / "b.bam"), want)


def test_levels_inflate_to_the_same_stream(spoiled, tmp_path):
    import sambamba_amd
    path, _, want, _ = spoiled
    sizes = {}
    for level in (0, 9):
        out = str(tmp_path / ("l%d.bam" % level))
        r = cli(["-l", str(level), path, out])
        assert r.returncode == 0, r.stderr
        check_file(out, want)
        sizes[level] = os.path.getsize(out)
    assert sizes[0] > len(want) > sizes[9]
    sambamba_amd.fixbins(path, str(tmp_path / "api0.bam"), level=0)
    check_file(str(tmp_path / "api0.bam"), want)


def test_empty_bam(tmp_path):
    import sambamba_amd
    path = str(tmp_path / "empty.bam")
    bc.write(path, [])
    out = str(tmp_path / "o.bam")
    st = sambamba_amd.fixbins(path, out)
    assert (st["n_records"], st["n_bins_changed"]) == (0, 0)
    check_file(out, inflate(path))


def test_failures_leave_no_output(spoiled, tmp_path):
    import sambamba_amd
    path = spoiled[0]
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.fixbins(path, path)
    assert ei.value.code == -1 and "would overwrite the input" in ei.value.msg
    r = cli([path, path])
    assert (r.returncode, r.stderr) == (1, ("sbx-fixbins: the output would overwrite the input %s\n" % path).encode())
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.fixbins(path, str(tmp_path / "x.bam"), level=10)
    assert ei.value.code == -1
    # a CIGAR count that runs past the record's block_size
    recs, _ = bc.records()
    broken = bytearray(recs[50])
    struct.pack_into("<H", broken, 16, 4000)
    bad = str(tmp_path / "bad.bam")
    # (bamgen.write_bam reads the CIGAR of what it writes: the file is put together here)
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bc.REFS)
    stream = bamgen.bam_header(text, bc.REFS) + b"".join(recs[:50]) + bytes(broken) + b"".join(recs[51:100])
    with open(bad, "wb") as fh:
        fh.write(bamgen.bgzf_block(stream) + bamgen.EOF_BLOCK)
    out = str(tmp_path / "bad.out.bam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.fixbins(bad, out)
    assert ei.value.code == -3
    with pytest.raises(sambamba_amd.SbxError):
        sambamba_amd.fixbins(str(tmp_path / "missing.bam"), out)
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "x.bam"))


def test_abi_sizeof_fixbins_stats():
    import sambamba_amd
    from sambamba_amd._lib import FixbinsStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_fixbins_stats") == C.sizeof(FixbinsStats) == 5 * 8 + 2 * 4 + 6 * 8
