"""`sambamba flagstat` on the device (sbx_flagstat, K8 flagstat.hip) through the Python API and the `sbx-flagstat` CLI, against
the pure-Python restatement of flagstat.d (tests/flagstat_ref.py): the reference's fixtures, every flag value, records that
straddle BGZF blocks and batches, a synthetic BAM, and the error cases.

tests/golden/match_mates.bam is a verbatim copy of the reference test-suite's test/match_mates.bam (test data, 1.1 KB):
`SO:unsorted`, no .bai, and the only fixture with QC-failed and secondary records (14 + 8)."""
import os
import subprocess

import pytest

from tests import bamgen
from tests import flagstat_ref as ref
from tests.util import GOLDEN, gen_bam, scan_bgzf

pytestmark = pytest.mark.gpu

REFS = [("c1", 100000), ("c2", 50000)]
UNSORTED = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:50000\n"


def cli(args, env=None):
    from sambamba_amd import flagstat_cli_path
    return subprocess.run([flagstat_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def check(path, want=None):
    """API and CLI (plain and -b) against the restatement; returns the counts."""
    import sambamba_amd
    want = want or ref.count(path)
    assert sambamba_amd.flagstat(path) == want
    for args, tab in (([path], False), (["-b", path], True)):
        r = cli(args)
        assert r.returncode == 0, r.stderr
        assert r.stdout.decode() == ref.text(want, tabular=tab)
    return want


def _all_flag_records():
    """Every flag value x next_refID in {same, other, -1} x mapq in {0, 4, 5, 60}, then unplaced reads (refID -1) at the end."""
    recs = []
    for flag in range(4096):
        for k, next_ref in enumerate((0, 1, -1)):
            for mapq in (0, 4, 5, 60):
                pos = (flag * 12 + k * 4) % 90000
                recs.append(bamgen.make_record(0, pos, "6M", "ACGTAC", 30, name="f%x" % flag, mapq=mapq, flag=flag,
                                               next_ref=next_ref, next_pos=pos))
    for flag in range(0, 4096, 37):
        recs.append(bamgen.make_record(-1, -1, "", "ACGT", 30, name="u%x" % flag, mapq=0, flag=flag | 0x4, next_ref=-1))
    return recs


@pytest.fixture(scope="module")
def flags_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("flagstat")
    recs = _all_flag_records()
    files = {}
    info = bamgen.write_bam(str(d / "all.bam"), REFS, recs, text=UNSORTED, write_index=False)
    files["all"] = str(d / "all.bam")
    starts = [r[3] for r in info["records"]]
    cuts = [s + 3 for s in starts[::97]] + [s + 30 for s in starts[50::211]]
    bamgen.write_bam(str(d / "cuts.bam"), REFS, recs, text=UNSORTED, cuts=cuts, write_index=False)
    files["cuts"] = str(d / "cuts.bam")
    bamgen.write_bam(str(d / "tiny.bam"), REFS, recs, text=UNSORTED, block_size=300, write_index=False)
    files["tiny"] = str(d / "tiny.bam")
    bamgen.write_bam(str(d / "levels.bam"), REFS, recs, text=UNSORTED, block_size=1000, levels=[0, 1, 9, 0, 6], write_index=False)
    files["levels"] = str(d / "levels.bam")
    return d, files, info, ref.count(files["all"])


def test_reference_fixtures():
    for name in ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates"):
        check(os.path.join(GOLDEN, name + ".bam"))


def test_match_mates_has_both_halves():
    """The unsorted, unindexed fixture: QC-failed and secondary records in both columns."""
    path = os.path.join(GOLDEN, "match_mates.bam")
    assert not os.path.exists(path + ".bai")
    got = check(path)
    assert got["reads"] == (14, 8) and got["secondary"] == (14, 8)


def test_every_flag_value(flags_dir):
    _, files, _, want = flags_dir
    assert want["reads"][0] + want["reads"][1] == 4096 * 12 + len(range(0, 4096, 37))
    assert all(v[0] > 0 and v[1] > 0 for v in want.values())
    check(files["all"], want)


@pytest.mark.parametrize("kind", ["cuts", "tiny", "levels"])
def test_records_straddling_blocks(flags_dir, kind):
    _, files, _, want = flags_dir
    check(files[kind], want)


@pytest.mark.parametrize("kind", ["all", "tiny"])
def test_batches_count_every_record_once(flags_dir, kind, monkeypatch):
    import sambamba_amd
    _, files, info, want = flags_dir
    path = files[kind]
    batch = str(info["stream_len"] // 12)
    r = cli([path], env={"SBX_INDEX_BATCH_BYTES": batch, "SBX_TIMING": "1"})
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == ref.text(want)
    line = [x for x in r.stderr.decode().splitlines() if x.startswith("[sbx] flagstat:")]
    assert len(line) == 1
    n_batches = int(line[0].split(" in ")[1].split(" batch")[0])
    assert n_batches >= 10, line[0]
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    assert sambamba_amd.flagstat(path) == want


def test_generated_bam(tmp_path):
    bam = gen_bam(str(tmp_path / "g.bam"), "chrA:2000000,chrB:1500000", coverage=12, seed=77)
    got = check(bam)
    # the generator's duplicates (2 %) and QC-failed pairs (0.5 %) fill both columns
    assert got["reads"][1] > 0 and got["dup"][0] > 0 and got["dup"][1] > 0 and got["pair_good"][1] > 0


def test_header_only(tmp_path):
    path = str(tmp_path / "empty.bam")
    bamgen.write_bam(path, REFS, [], text=UNSORTED, write_index=False)
    got = check(path)
    assert all(v == (0, 0) for v in got.values())
    assert "0 + 0 mapped (N/A:N/A)" in cli([path]).stdout.decode()


def _assert_fails(path, code):
    import sambamba_amd
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.flagstat(path)
    assert ei.value.code == code, ei.value
    r = cli([path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr


def test_truncated_and_corrupt(flags_dir, tmp_path):
    _, files, info, _ = flags_dir
    raw = open(files["all"], "rb").read()
    # a cut inside a BGZF block
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(raw[:len(raw) // 2])
    _assert_fails(cut, -3)
    # a cut at a block boundary inside a record: the record chain ends in the middle of a record
    _, co, _, _, oo, _ = scan_bgzf(files["all"])
    starts = {r[3] for r in info["records"]}
    k = next(k for k in range(len(co) // 2, len(co)) if int(oo[k]) not in starts)
    chopped = str(tmp_path / "chopped.bam")
    open(chopped, "wb").write(raw[:int(co[k]) - 18])
    _assert_fails(chopped, -3)
    # a deflate block of the reserved type in the middle of the file
    bad = str(tmp_path / "bad.bam")
    _, co, _, _, _, _ = scan_bgzf(files["levels"])
    b = bytearray(open(files["levels"], "rb").read())
    b[int(co[len(co) // 2])] = 0xFF
    open(bad, "wb").write(b)
    _assert_fails(bad, -3)


def test_missing_file(tmp_path):
    _assert_fails(str(tmp_path / "no_such.bam"), -2)


def test_cli_arguments(flags_dir):
    _, files, _, want = flags_dir
    r = cli([])
    assert r.returncode == 1 and r.stdout == b"" and b"Usage" in r.stderr
    path = os.path.join(GOLDEN, "match_mates.bam")
    plain = cli([path]).stdout
    assert plain == ref.text(ref.count(path)).encode()
    for args in (["-t", "4", path], [path, "-t", "4"], ["--nthreads=4", path], ["-p", path], [path, "-p", "-t4"],
                 [path, "--show-progress"]):
        r = cli(args)
        assert r.returncode == 0 and r.stdout == plain, args
    assert cli([path, "-b"]).stdout == cli(["--tabular", path]).stdout == ref.text(ref.count(path), tabular=True).encode()
