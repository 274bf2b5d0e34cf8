"""`sambamba markdup` on the device -- sbx_markdup: K10a ends, K10b pairing, K10c groups, K10d flags (markdup.hip) between the read
pass and the BGZF encoder -- through the Python API and the `sbx-markdup` CLI, against the pure-Python restatement of markdup.d
(tests/markdup_ref.py).  Every comparison is byte for byte on the INFLATED output; the file itself must end with the EOF block and
hold no block of more than 0xFF00 payload bytes."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import markdup_cases as mc
from tests import markdup_ref as ref
from tests.flagstat_ref import inflate
from tests.util import GOLDEN, scan_bgzf

pytestmark = pytest.mark.gpu

FIXTURES = ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates")


def cli(args, env=None):
    from sambamba_amd import markdup_cli_path
    return subprocess.run([markdup_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def check_file(path, want):
    """The BGZF file at `path` inflates to `want`, ends with the EOF block and has no payload above 0xFF00 bytes."""
    raw = open(path, "rb").read()
    assert raw[-28:] == bamgen.EOF_BLOCK
    _, _, _, isize, _, _ = scan_bgzf(path)
    assert all(int(x) <= 0xFF00 for x in isize)
    assert int(isize[-1]) == 0 and all(int(x) > 0 for x in isize[:-1])
    got = inflate(path)
    assert len(got) == len(want)
    assert got == want


def check(path, tmp_path, remove=False, level=-1, tag="o", env=None, stream=None):
    """API and CLI against the restatement; returns the API's stats."""
    import sambamba_amd
    stream = stream if stream is not None else inflate(path)
    out_api = str(tmp_path / (tag + ".api.bam"))
    st = sambamba_amd.markdup(path, out_api, remove_duplicates=remove, level=level, command_line="markdup from the test")
    want = ref.expected_stream(stream, remove, "markdup from the test")
    check_file(out_api, want)
    out_cli = str(tmp_path / (tag + ".cli.bam"))
    args = (["-r"] if remove else []) + (["-l", str(level)] if level != -1 else []) + [path, out_cli]
    r = cli(args, env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    check_file(out_cli, ref.expected_stream(stream, remove, "markdup " + " ".join(args)))
    text, _, _, recs = ref.split_stream(stream)
    dup, n_pairs, n_single, n_unmatched = ref.analyse(recs, text.decode())
    n_out = len(ref.split_stream(want)[3])
    assert (st["n_records_in"], st["n_records_out"]) == (len(recs), n_out)
    assert (st["n_end_pairs"], st["n_single_ends"], st["n_unmatched_pairs"], st["n_duplicates"]) == (n_pairs, n_single, n_unmatched, len(dup))
    assert st["stream_bytes"] == len(want) and st["compressed_bytes"] == os.path.getsize(out_api)
    lines = [x for x in r.stderr.decode().splitlines() if not x.startswith("[sbx]")]
    assert lines == ["finding positions of the duplicate reads in the file...", "  sorted %d end pairs" % n_pairs,
                     "     and %d single ends (among them %d unmatched pairs)" % (n_single, n_unmatched), "  found %d duplicates" % len(dup),
                     "removing duplicates..." if remove else "marking duplicates..."]
    if remove:       # -r counts: what is left is what carries no 0x400
        marked = sum(1 for r_ in ref.split_stream(ref.expected_stream(stream, False))[3] if struct.unpack_from("<H", r_, 18)[0] & 0x400)
        assert st["n_records_out"] == st["n_records_in"] - marked
    return st


def write(path, records, **kw):
    return bamgen.write_bam(str(path), mc.REFS, records, text=mc.TEXT, write_index=False, **kw)


@pytest.mark.parametrize("remove", [False, True])
def test_scenarios(tmp_path, remove):
    records, dups, _, counts = mc.scenarios()
    path = str(tmp_path / "scenarios.bam")
    write(path, records)
    st = check(path, tmp_path, remove=remove)
    # the literal counts of tests/markdup_cases.py, not the restatement's
    assert (st["n_end_pairs"], st["n_single_ends"], st["n_unmatched_pairs"], st["n_duplicates"]) == counts + (len(dups),) == (12, 23, 4, 18)
    assert st["n_records_in"] == len(records) and st["n_records_out"] == len(records) - (len(dups) + 2 if remove else 0)
    if not remove:
        names = mc.labels(records)
        out = ref.split_stream(inflate(str(tmp_path / "o.api.bam")))[3]
        assert {n for n, r in zip(names, out) if struct.unpack_from("<H", r, 18)[0] & 0x400} == dups | {"s15s#0", "s15x#0"}


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures(name, tmp_path):
    path = os.path.join(GOLDEN, name + ".bam")
    check(path, tmp_path)
    check(path, tmp_path, remove=True, tag="r")


@pytest.fixture(scope="module")
def random_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mdrandom")
    out = {}
    for seed, shuffled in ((1, False), (2, True)):
        records = mc.random_records(20000, seed, shuffled)
        path = str(d / ("r%d.bam" % seed))
        info = write(path, records)
        out[seed] = (path, records, info, inflate(path))
    return out


@pytest.mark.parametrize("seed", [1, 2])
def test_random_differential(random_files, seed, tmp_path):
    path, records, _, stream = random_files[seed]
    dup = ref.duplicates(records, mc.TEXT)
    assert 0.05 * len(records) <= len(dup) <= 0.95 * len(records)          # no all-or-nothing output can pass
    check(path, tmp_path, stream=stream)
    check(path, tmp_path, remove=True, tag="r", stream=stream)


def _big_group(kind):
    """Groups larger than a radix tile (4096) and an offsets tile (2048), the unique top score in the middle."""
    n, recs = 5000, []
    for i in range(n):
        q = 40 if i == n // 2 else 30 - (i % 3)
        if kind == "pairs":
            recs += [mc.rec("p%05d" % i, 0, 1000, flag=mc.F1, qual=q), mc.rec("p%05d" % i, 0, 1300, flag=mc.R2, qual=q)]
        else:
            recs.append(mc.rec("f%05d" % i, 0, 1310, "10M", flag=0x10, qual=q))
    if kind == "fragments_at_end2":
        recs[n // 3:n // 3] = [mc.rec("P", 0, 900, flag=mc.F1), mc.rec("P", 0, 1310, flag=mc.R2)]
    return recs


@pytest.mark.parametrize("kind", ["fragments", "pairs", "fragments_at_end2"])
def test_groups_larger_than_a_tile(kind, tmp_path):
    records = _big_group(kind)
    path = str(tmp_path / "big.bam")
    write(path, records)
    st = check(path, tmp_path)
    # by hand: all but the one best fragment / pair; with a pair end at the key every fragment
    assert st["n_duplicates"] == {"fragments": 4999, "pairs": 2 * 4999, "fragments_at_end2": 5000}[kind]
    names = mc.labels(records)
    out = ref.split_stream(inflate(str(tmp_path / "o.api.bam")))[3]
    clean = {n for n, r in zip(names, out) if not struct.unpack_from("<H", r, 18)[0] & 0x400}
    assert clean == {"fragments": {"f02500#0"}, "pairs": {"p02500#0", "p02500#1"}, "fragments_at_end2": {"P#0", "P#1"}}[kind]


def test_forced_hash_runs(tmp_path, monkeypatch):
    import sambamba_amd
    records = [r for r in mc.random_records(3000, 5, True) if struct.unpack_from("<H", r, 18)[0] & 1][:2000]
    path = str(tmp_path / "h.bam")
    write(path, records)
    plain = str(tmp_path / "plain.bam")
    sambamba_amd.markdup(path, plain)
    want = ref.expected(path)
    check_file(plain, want)
    monkeypatch.setenv("SBX_MARKDUP_HASH_BITS", "4")
    forced = str(tmp_path / "forced.bam")
    st = sambamba_amd.markdup(path, forced)
    check_file(forced, want)
    assert inflate(forced) == inflate(plain) and st["n_end_pairs"] > 300
    r = cli([path, str(tmp_path / "forced.cli.bam")], env={"SBX_MARKDUP_HASH_BITS": "4"})
    assert r.returncode == 0, r.stderr
    assert ref.split_stream(inflate(str(tmp_path / "forced.cli.bam")))[3] == ref.split_stream(want)[3]


def test_batches_give_the_same_output(random_files, tmp_path, monkeypatch):
    import sambamba_amd
    path, _, info, stream = random_files[2]
    want = ref.expected_stream(stream)
    batch = str(info["stream_len"] // 4)
    out = str(tmp_path / "b.bam")
    r = cli([path, out], env={"SBX_INDEX_BATCH_BYTES": batch, "SBX_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    line = [x for x in r.stderr.decode().splitlines() if x.startswith("[sbx] markdup:")]
    assert len(line) == 1
    fields = dict(kv.split("=") for kv in line[0].split("(")[0].split()[2:])
    assert int(fields["n_batches"]) >= 3, line[0]
    assert ref.split_stream(inflate(out))[3] == ref.split_stream(want)[3]
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    out2 = str(tmp_path / "b2.bam")
    st = sambamba_amd.markdup(path, out2)
    assert st["n_batches"] >= 3
    check_file(out2, want)


def test_records_straddling_blocks(random_files, tmp_path):
    _, records, info, _ = random_files[1]
    records = records[:6000]
    starts = [r[3] for r in info["records"][:6000]]
    cuts = [s + 3 for s in starts[::97]] + [s + 19 for s in starts[50::211]] + [s + 40 for s in starts[20::301]]
    path = str(tmp_path / "cuts.bam")
    write(path, records, cuts=cuts)
    check(path, tmp_path)
    tiny = str(tmp_path / "tiny.bam")
    write(tiny, records[:3000], block_size=300)
    check(tiny, tmp_path, tag="t")


def test_levels_inflate_to_the_same_stream(random_files, tmp_path):
    import sambamba_amd
    path, _, _, stream = random_files[1]
    want = ref.expected_stream(stream)
    sizes = {}
    for level in (0, 1, 6):
        out = str(tmp_path / ("l%d.bam" % level))
        sambamba_amd.markdup(path, out, level=level)
        check_file(out, want)
        sizes[level] = os.path.getsize(out)
    assert sizes[0] > sizes[1] >= sizes[6]
    r = cli(["-l", "1", path, str(tmp_path / "c1.bam")])
    assert r.returncode == 0 and os.path.getsize(str(tmp_path / "c1.bam")) < sizes[0]


def test_degenerate_files(tmp_path):
    empty = str(tmp_path / "empty.bam")
    write(empty, [])
    st = check(empty, tmp_path, tag="e")
    assert st["n_records_out"] == 0 and st["n_duplicates"] == 0
    check(empty, tmp_path, remove=True, tag="er")
    unmapped = str(tmp_path / "unmapped.bam")
    write(unmapped, [bamgen.make_record(-1, -1, "", "ACGT", 30, name="u%d" % i, flag=0x4 | (0x400 if i % 3 == 0 else 0)) for i in range(700)])
    st = check(unmapped, tmp_path, tag="u")
    assert st["n_duplicates"] == st["n_single_ends"] == 0 and st["n_records_out"] == 700
    frags = str(tmp_path / "frags.bam")
    write(frags, [mc.rec("f%d" % i, i % 2, 100 + (i % 7), flag=0x10 if i % 5 == 0 else 0, qual=20 + i % 4) for i in range(900)])
    st = check(frags, tmp_path, tag="f")
    assert st["n_end_pairs"] == 0 and st["n_single_ends"] == 900 and 0 < st["n_duplicates"] < 900
    check(frags, tmp_path, remove=True, tag="fr")


def _assert_fails(path, code, tmp_path):
    import sambamba_amd
    out = str(tmp_path / "fail.bam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.markdup(path, out)
    assert ei.value.code == code, ei.value
    assert not os.path.exists(out)
    r = cli([path, out])
    assert r.returncode == 1 and r.stdout == b"" and b"\nsbx-markdup: " in r.stderr
    assert not os.path.exists(out)


def test_missing_truncated_and_corrupt(random_files, tmp_path):
    path, _, _, _ = random_files[1]
    _assert_fails(str(tmp_path / "no_such.bam"), -2, tmp_path)
    raw = open(path, "rb").read()
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(raw[:len(raw) // 2])
    _assert_fails(cut, -3, tmp_path)
    _, co, _, _, _, _ = scan_bgzf(path)
    bad = str(tmp_path / "bad.bam")
    b = bytearray(raw)
    b[int(co[len(co) // 2])] = 0xFF
    open(bad, "wb").write(b)
    _assert_fails(bad, -3, tmp_path)


def test_cigar_count_overruns_the_record(tmp_path):
    """Built as data: n_cigar_op says 4000 operations in a record of 60-odd bytes.  Run once."""
    good = mc.rec("ok", 0, 100)
    bad = bytearray(mc.rec("bad", 0, 200))
    struct.pack_into("<H", bad, 16, 4000)
    path = str(tmp_path / "overrun.bam")
    # (bamgen.write_bam reads the CIGAR of what it writes: the file is put together here)
    stream = bamgen.bam_header(mc.TEXT, mc.REFS) + good + bytes(bad) + good
    open(path, "wb").write(bamgen.bgzf_block(stream) + bamgen.EOF_BLOCK)
    _assert_fails(path, -3, tmp_path)


def test_reference_id_out_of_range(tmp_path):
    path = str(tmp_path / "badref.bam")
    write(path, [mc.rec("a", 0, 10), mc.rec("b", 2, 10)])
    _assert_fails(path, -3, tmp_path)


def test_output_must_not_be_the_input(tmp_path):
    import sambamba_amd
    path = str(tmp_path / "in.bam")
    write(path, mc.scenarios()[0])
    before = open(path, "rb").read()
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.markdup(path, path)
    assert ei.value.code == -1                  # SBX_EINVAL
    r = cli([path, str(tmp_path / "." / "in.bam")])
    assert r.returncode == 1 and r.stderr.startswith(b"sbx-markdup: ")
    assert open(path, "rb").read() == before


def test_abi_sizeof_markdup_stats():
    import sambamba_amd
    from sambamba_amd._lib import MarkdupStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_markdup_stats") == C.sizeof(MarkdupStats) == 9 * 8 + 2 * 4 + 8 * 8
