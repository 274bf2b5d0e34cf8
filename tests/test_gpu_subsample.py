"""`sbx-subsample` on the device (sbx_subsample: K22a marks, K22b scans, K22c judges, K21 writes) against the Python restatement of its
definition (tests/subsample_ref.py).  Files are generated with tests/bamgen.py; every output is compared record for record with the
restatement and the stats with its counts.  The shapes are the smallest at which a kernel can go wrong: a pile on one position, a
verdict that only the end (or only the start) of a span decides, records that must not count, spans at the edges of references,
slots at the edges of the scan's tiles and more tiles than one round of the tile-sum scan takes, read batches and output windows cut
through records and through the patched flag, shuffled input."""
import filecmp
import os
import random
import re
import struct
import subprocess

import pytest

from tests import bamgen
from tests import subsample_ref as ref
from tests.util import ROOT

pytestmark = pytest.mark.gpu

PIECE = 0xFF00
CL = "subsample --type fasthash --max-cov N"
TILE = int(re.search(r"constexpr uint32_t kCovTile = (\d+);", open(os.path.join(ROOT, "sambamba_amd", "csrc", "subsample_core.hpp")).read()).group(1))
HOOKS = ("SBX_INDEX_BATCH_BYTES", "SBX_STREAM_WINDOW_BYTES", "SBX_BGZF_PIECE_BLOCKS")


def rec(ref_id, pos, cigar, name, flag=0):
    return bamgen.make_record(ref_id, pos, cigar, "ACGTAC", 30, name=name, flag=flag)


def header_text(refs, pad=None):
    text = "@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    return text if pad is None else text + "@CO\t" + "x" * pad + "\n"


def check(tmp_path, refs, recs, max_cov, remove, tag="o", text=None, block_size=0xFF00, **kw):
    """writes the records, runs subsample, compares output and counts with the restatement; (stats, records written, verdicts)"""
    import sambamba_amd
    path, out = str(tmp_path / (tag + ".in.bam")), str(tmp_path / (tag + ".out.bam"))
    text = text or header_text(refs)
    bamgen.write_bam(path, refs, recs, text=text, write_index=False, block_size=block_size)
    st = sambamba_amd.subsample(path, out, max_cov, remove=remove, command_line=CL, **kw)
    got_text, lns, got = ref.read_bam(out)
    assert lns == [ln for _, ln in refs]
    want, counts = ref.subsample(recs, lns, max_cov, remove, TILE)
    print("%s: %s" % (tag, " ".join("%s=%s" % (k, st[k]) for k in ("n_records", "n_counted", "n_over", "n_dropped", "n_written", "max_cov_seen",
                                                                   "n_batches", "n_windows", "ms_mark", "ms_scan", "ms_verdict"))))
    assert len(got) == len(want) and got == want
    for k, v in counts.items():
        assert st[k] == v, (k, st[k], v)
    assert got_text == sambamba_amd.markdup_header_text(text, CL) and "SO:coordinate" in got_text and "CL:" + CL in got_text
    assert st["compressed_bytes"] == os.path.getsize(out) and st["n_windows"] >= 1
    return st, got, ref.verdicts(recs, lns, max_cov)


def pile(n=40, pos=100, cigar="50M"):
    return [rec(0, pos, cigar, "p%03d" % k, flag=(0x10 if k % 3 == 0 else 0)) for k in range(n)]


@pytest.mark.parametrize("remove", [True, False])
def test_pile(tmp_path, remove):
    refs = [("chr1", 1000)]
    st, got, v = check(tmp_path, refs, pile(), 10, remove)
    assert st["max_cov_seen"] == 40 and st["n_over"] == 40 and 0 < st["n_dropped"] < 40
    assert st["n_written"] == (40 - st["n_dropped"] if remove else 40)
    if not remove:
        assert sum(ref.flag_of(r) & 0x200 != 0 for r in got) == st["n_dropped"]


def name_with(dropped_at, max_cov, prefix):
    """a name that is dropped at coverage dropped_at under max_cov (kept at any coverage <= max_cov whatever it is)"""
    for k in range(10000):
        name = "%s%d" % (prefix, k)
        if not ref.keeps(ref.name_hash32(name.encode()), dropped_at, max_cov):
            return name
    raise AssertionError("no such name")


@pytest.mark.parametrize("which", ["end", "start"])
def test_one_end_of_the_span_decides(tmp_path, which):
    """A covers 100 positions and meets a pile of 20 only at its last (first) ten: its coverage is 1 at one end and 21 at the other,
    and its name is one that 21 drops under a cap of 5"""
    refs = [("chr1", 1000)]
    name = name_with(21, 5, "A")
    if which == "end":
        recs = [rec(0, 0, "100M", name)] + [rec(0, 90, "30M", "q%02d" % k) for k in range(20)]
        a = 0
    else:
        recs = [rec(0, 0, "30M", "q%02d" % k) for k in range(20)] + [rec(0, 20, "100M", name)]
        a = 20
    cov = ref.coverage(recs, [1000])[0]
    assert (cov[0], cov[99]) == (1, 21) if which == "end" else (cov[20], cov[119]) == (21, 1)
    st, got, v = check(tmp_path, refs, recs, 5, True)
    assert v[a] == (True, 21, True) and ref.name_of(recs[a]) not in [ref.name_of(r) for r in got]


def test_uncounted_records_are_kept_unpatched_and_add_no_coverage(tmp_path):
    refs = [("chr1", 1000)]
    odd = [rec(0, 100, "50M", "unmapped", flag=0x4), rec(0, 100, "50M", "qcfail", flag=0x200), rec(0, 100, "50M", "dup", flag=0x400),
           rec(0, 100, "50M", "dupqc", flag=0x600 | 0x10), rec(-1, 120, "50M", "noref"), rec(-1, -1, "", "nothing", flag=0x4)]
    recs = pile(20) + odd[:4] + pile(20)[10:] + odd[4:]
    for remove in (True, False):
        st, got, v = check(tmp_path, refs, recs, 10, remove, tag="r%d" % remove)
        assert st["max_cov_seen"] == 30 and st["n_counted"] == 30 and 0 < st["n_dropped"] < 30
        for r in odd:
            assert r in got


def test_reference_edges(tmp_path):
    """spans that end at LN (and would pass it) of reference 0, a record at position 0 of reference 1 that must see none of them,
    positions at and behind LN, CIGARs without reference bases, a reference of length 0"""
    refs = [("a", 200), ("b", 300), ("z", 0), ("c", 50)]
    recs = [rec(0, 150, "50M", "e%02d" % k) for k in range(12)] + [rec(0, 190, "50M", "f%d" % k) for k in range(3)]
    recs += [rec(0, 199, "1M", "last"), rec(0, 200, "10M", "atln"), rec(0, 250, "10M", "behind")]
    recs += [rec(1, 0, "10M", "first")] + [rec(1, 100, "5I", "i%d" % k) for k in range(8)] + [rec(1, 100, "", "n%d" % k) for k in range(4)]
    recs += [rec(1, 299, "100M", "tail"), rec(2, 0, "5M", "zero"), rec(3, 49, "10M", "c49"), rec(3, 0, "50M", "c0")]
    st, got, v = check(tmp_path, refs, recs, 3, False)
    by_name = {ref.name_of(r).decode(): x for r, x in zip(recs, v)}
    assert by_name["first"] == (True, 1, False) and by_name["last"][1] == 16 and by_name["e00"][1] == 16
    assert by_name["atln"] == by_name["behind"] == by_name["zero"] == (False, 0, False)
    assert by_name["i0"][1] == 12 and by_name["tail"] == (True, 1, False) and by_name["c49"][1] == 2
    assert st["max_cov_seen"] == 16 and st["n_dropped"] > 0


def test_scan_tiles(tmp_path):
    """references of kCovTile - 1, kCovTile and kCovTile + 1 positions and one of more than 1024 tiles; piles that cross tile edges
    and single records right behind the edges, which must see a coverage of 1"""
    T = TILE
    refs = [("t0", T - 1), ("t1", T), ("t2", T + 1), ("big", 1030 * T + 100)]
    base = ref.slot_bases([ln for _, ln in refs])
    assert base[:4] == [0, T, 2 * T + 1, 3 * T + 3] and -(-base[-1] // T) > 1024 + 4
    recs = [rec(0, T - 6, "3M", "a%d" % k) for k in range(4)] + [rec(0, T - 3, "5M", "b%d" % k) for k in range(5)] + [rec(0, T - 2, "1M", "c")]
    # reference 1 owns slots T .. 2T: a probe on the first slot of tile 1, a pile whose -1 falls on the first slot of tile 2
    recs += [rec(1, 0, "1M", "probe1")] + [rec(1, T - 2, "2M", "d%d" % k) for k in range(6)]
    recs += [rec(2, 0, "4M", "probe2"), rec(2, T, "1M", "probe2b")]
    big = []
    for tile in (5, 6, 1024, 1025, 1032):
        edge = tile * T - base[3]                        # the position of `big` whose slot is the first of that tile
        big += [rec(3, edge - 5, "10M", "x%d_%d" % (tile, k)) for k in range(6)]                 # slots edge - 5 .. edge + 4
        big += [rec(3, edge - 1, "2M", "y%d" % tile)]                                            # slots T * tile - 1 and T * tile
        big += [rec(3, edge + 20, "3M", "probe%d" % tile)]
    recs += big + [rec(3, 1030 * T + 99, "5M", "end")]
    st, got, v = check(tmp_path, refs, recs, 2, False)
    by_name = {ref.name_of(r).decode(): x for r, x in zip(recs, v)}
    for name in ["probe1", "probe2", "probe2b", "end"] + ["probe%d" % t for t in (5, 6, 1024, 1025, 1032)]:
        assert by_name[name] == (True, 1, False), name
    assert by_name["y1024"][1] == 7 and by_name["d0"][1] == 6 and by_name["c"][1] == 6 and st["max_cov_seen"] == 7
    assert st["cov_array_bytes"] == -(-base[-1] // T) * T * 4 and st["n_dropped"] > 0


def many_records(seed=5, n=3000):
    rng = random.Random(seed)
    spec = sorted((rng.randrange(0, 5000), rng.choice(("36M", "10M2I20M", "5S30M", "20M300N10M", "12M3D12M"))) for _ in range(n))
    return [rec(0, pos, cigar, "r%05d" % k, flag=(0x400 if k % 50 == 0 else 0x10 if k % 2 else 0)) for k, (pos, cigar) in enumerate(spec)]


def hooked(monkeypatch, on):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    if on:
        monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", "20000")
        monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", "1")
        monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")


@pytest.mark.parametrize("remove", [True, False])
def test_batches_and_windows(tmp_path, monkeypatch, remove):
    """both read passes in several batches, the output through several windows of one piece: the file of the run without hooks, byte
    for byte.  Without -r the header is padded so that byte 18 of a record that is dropped is the last byte of the first window."""
    import sambamba_amd
    refs = [("chr1", 100000)]
    recs = many_records(n=4000)
    lns = [100000]
    text = header_text(refs, 100)
    if not remove:
        v = ref.verdicts(recs, lns, 50)
        off, offs = 0, []
        for r in recs:
            offs.append(off)
            off += len(r)
        hlen = len(bamgen.bam_header(sambamba_amd.markdup_header_text(text, CL), refs))
        k = next(i for i, o in enumerate(offs) if v[i][2] and PIECE - 2000 <= hlen + o < PIECE - 300)
        text = header_text(refs, 100 + (PIECE - 1) - (hlen + offs[k] + 18))
        hlen = len(bamgen.bam_header(sambamba_amd.markdup_header_text(text, CL), refs))
        assert hlen + offs[k] + 18 == PIECE - 1 and v[k][2]                   # (checked on the CPU)
    hooked(monkeypatch, False)
    st_a, got, _ = check(tmp_path, refs, recs, 50, remove, tag="plain", text=text, block_size=700)
    hooked(monkeypatch, True)
    st_b, _, _ = check(tmp_path, refs, recs, 50, remove, tag="hooked", text=text, block_size=700)
    hooked(monkeypatch, False)
    assert filecmp.cmp(str(tmp_path / "plain.out.bam"), str(tmp_path / "hooked.out.bam"), shallow=False)
    assert st_b["n_batches"] >= 6 and st_b["n_batches"] % 2 == 0 and st_b["window_bytes"] == PIECE
    assert st_b["n_windows"] == -(-st_b["stream_bytes"] // PIECE) >= 3 and st_b["n_pack_launches"] > st_b["n_windows"]
    assert 500 < st_b["n_dropped"] < 2500 and st_a["n_batches"] == 2 and st_a["n_windows"] == 1


def test_order_independence(tmp_path):
    refs = [("chr1", 100000)]
    recs = many_records(seed=9, n=1500)
    shuffled = list(recs)
    random.Random(1).shuffle(shuffled)
    _, got_a, _ = check(tmp_path, refs, recs, 6, False, tag="sorted")
    st, got_b, _ = check(tmp_path, refs, shuffled, 6, False, tag="shuffled")
    assert got_a != got_b and sorted(got_a) == sorted(got_b) and st["n_dropped"] > 100


@pytest.mark.parametrize("max_cov", [40, 41, (1 << 31) - 1])
def test_cap_at_or_above_the_largest_coverage(tmp_path, max_cov):
    refs = [("chr1", 1000)]
    recs = pile() + [rec(0, 500, "10M", "far")]
    for remove in (True, False):
        st, got, _ = check(tmp_path, refs, recs, max_cov, remove, tag="r%d" % remove)
        assert got == recs and st["n_dropped"] == 0 and st["n_over"] == 0 and st["max_cov_seen"] == 40 and st["n_written"] == 41


def test_failures_leave_no_output(tmp_path, monkeypatch):
    import sambamba_amd
    refs = [("chr1", 100000)]
    recs = many_records(seed=3, n=1000)
    broken = bytearray(recs[-3])
    struct.pack_into("<H", broken, 16, 4000)             # a CIGAR count that runs past block_size, in the last batch
    stream = bamgen.bam_header(header_text(refs), refs) + b"".join(recs[:-3]) + bytes(broken) + b"".join(recs[-2:])
    bad = str(tmp_path / "bad.bam")
    with open(bad, "wb") as fh:
        fh.write(b"".join(bamgen.bgzf_block(stream[o:o + 700]) for o in range(0, len(stream), 700)) + bamgen.EOF_BLOCK)
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", "20000")
    out = str(tmp_path / "bad.out.bam")
    for remove in (True, False):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.subsample(bad, out, 10, remove=remove)
        assert ei.value.code == -3 and "malformed BAM record" in ei.value.msg and not os.path.exists(out)
    monkeypatch.delenv("SBX_INDEX_BATCH_BYTES")
    # refused through the command line: more than one input, the output is the input
    good = str(tmp_path / "good.bam")
    bamgen.write_bam(good, refs, recs[:50], write_index=False)
    cli = sambamba_amd.subsample_cli_path()
    r = subprocess.run([cli, "--type", "fasthash", "--max-cov", "5", "-o", out, good, good], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"more than one input file is not supported" in r.stderr and not os.path.exists(out)
    before = open(good, "rb").read()
    r = subprocess.run([cli, "--type", "fasthash", "--max-cov", "5", "-o", good, good], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stderr == b"sbx-subsample: Input file can not be same as output file " + good.encode() + b"\n"
    assert open(good, "rb").read() == before
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.subsample(good, good, 5)
    assert ei.value.code == -1 and open(good, "rb").read() == before


def test_index_of_the_output(tmp_path):
    import sambamba_amd
    refs = [("chr1", 100000)]
    st, got, _ = check(tmp_path, refs, many_records(seed=2, n=800), 8, True, index=True)
    out = str(tmp_path / "o.out.bam")
    assert st["n_dropped"] > 0 and os.path.exists(out + ".bai")
    sambamba_amd.build_index(out, str(tmp_path / "again.bai"))
    assert filecmp.cmp(out + ".bai", str(tmp_path / "again.bai"), shallow=False)


def test_cli_end_to_end_with_the_timing_line(tmp_path):
    import sambamba_amd
    refs = [("chr1", 1000)]
    recs = pile()
    path, out = str(tmp_path / "in.bam"), str(tmp_path / "cli.bam")
    bamgen.write_bam(path, refs, recs, write_index=False)
    args = ["--type=fasthash", "--max-cov", "10", path, "-r", "-l", "1", "-o", out]
    r = subprocess.run([sambamba_amd.subsample_cli_path()] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, SBX_TIMING="1"))
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    lines = [l for l in r.stderr.decode().splitlines() if l.startswith("[sbx] subsample:")]
    want, counts = ref.subsample(recs, [1000], 10, True, TILE)
    assert len(lines) == 1 and " n_dropped=%d " % counts["n_dropped"] in lines[0] and " max_cov_seen=40 " in lines[0]
    text, _, got = ref.read_bam(out)
    assert got == want and text == sambamba_amd.markdup_header_text(header_text(refs), "subsample " + " ".join(args))
    assert not os.path.exists(out + ".bai")
