"""The indexed `view` on the device -- sbx_view_run_indexed: the runs the .bai names for the regions, the planner of
view_index_core.hpp, K12c's order check and the three sinks over the planned batches -- through the Python API (use_index) and the
`sbx-iview` CLI.  Every case is compared with the restatements the whole-file tests use (tests/view_ref.py, tests/sam_ref.py), byte
for byte with the same request in OFF mode, and its cost with the blocks tests/view_index_ref.py derives from the .bai.  The file has
BGZF blocks of 600 bytes, three contigs (one without records) and unplaced reads; every case runs with the default batch size and
with SBX_INDEX_BATCH_BYTES small enough to cut the longer runs into many pieces."""
import os
import shutil
import subprocess

import pytest

from tests import bamgen, sam_ref
from tests import view_index_ref as ixref
from tests import view_ref as ref
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream
from tests.test_gpu_sort import check_file

pytestmark = pytest.mark.gpu

REFS = [("chr1", 3000000), ("chr2", 100000), ("chr3", 50000)]
BLOCK = 600
SMALL_BATCH = "4096"            # seven blocks: the run of a dense 16 kbp window (about 85 blocks) falls into a dozen pieces
BATCHES = pytest.mark.parametrize("batch", [None, SMALL_BATCH], ids=["default", "small_batches"])


def rec(ref, pos, cigar, name, flag=0, mapq=30):
    n = sum(k for op, k in bamgen.parse_cigar(cigar) if op in "MIS=X")
    return bamgen.make_record(ref, pos, cigar, "ACGT" * (n // 4) + "A" * (n % 4), 30, name=name, flag=flag, mapq=mapq)


def main_records(unplaced=True):
    """(records in file order, {group name: index of its first record})"""
    recs, groups = [], {}

    def group(name, rs):
        groups[name] = len(recs)
        recs.extend(rs)

    # covers chr1:100000-1100020 and lies in bin 9: it overlaps every region up to there, and the linear index of all those
    # windows points at it
    group("far", [rec(0, 100000, "10M1000000N10M", "far")])
    group("dense", [rec(0, 200000 + 40 * k, "50M", "a%04d" % k, mapq=20 + k % 30, flag=(1024 if k % 7 == 0 else 0))
                    for k in range(3000)])                                          # 200000 .. 319960
    group("zero", [rec(0, 400000, "", "zero_at_start"), rec(0, 400010, "20M", "z_plain"), rec(0, 400050, "", "zero_inside")])
    # behind the end of `far`, each group in a 16 kbp window of its own
    group("g1", [rec(0, 1190000 + 10 * k, "25M", "g1_%02d" % k) for k in range(12)])
    group("f1", [rec(0, 1210000 + 10 * k, "25M", "f1_%02d" % k) for k in range(4)])   # less than one block
    group("g2", [rec(0, 1230000 + 10 * k, "25M", "g2_%02d" % k) for k in range(12)])
    group("f2", [rec(0, 1250000 + 10 * k, "25M", "f2_%02d" % k) for k in range(18)])  # between two and three blocks
    group("g3", [rec(0, 1270000 + 10 * k, "25M", "g3_%02d" % k) for k in range(12)])
    group("late", [rec(0, 2000000 + 40 * k, "30M", "l%03d" % k) for k in range(100)])
    group("chr3", [rec(2, 100 + 30 * k, "40M", "d%03d" % k) for k in range(100)])    # 100 .. 3070: one window
    if unplaced:
        group("unplaced", [rec(-1, -1, "", "u%02d" % k, flag=4, mapq=0) for k in range(40)])
    return recs, groups


def write(path, recs, cuts=None, refs=REFS):
    import sambamba_amd
    info = bamgen.write_bam(path, refs, recs, block_size=BLOCK, cuts=cuts, write_index=False)
    sambamba_amd.build_index(path, path + ".bai")
    return info


def write_main(path, unplaced=True):
    recs, groups = main_records(unplaced)
    # record offsets do not depend on the cuts: a first pass gives them
    offs = []
    o = len(bamgen.bam_header("@HD\tVN:1.6\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS), REFS))
    for r in recs:
        offs.append(o)
        o += len(r)
    write(path, recs, cuts=main_cuts(groups, offs))
    return recs, groups, offs


FIRST_OF_WINDOW_14, LAST_OF_RUN_14 = 734, 1143      # dense records: 229360 reaches into window 14 first, 245720 is the last in bin 586


def main_cuts(groups, offs):
    """Block boundaries at the starts of f1, g2, f2, g3 (so the gaps between the runs of g1, g2, g3 are whole blocks: one and three);
    one byte behind the start of the first record of the `zero` window (its chunk begins at the last byte of a block); and inside the
    first and the last record of the run the .bai names for window 14 of chr1 (both straddle a block boundary)."""
    d0 = groups["dense"]
    return ([offs[groups[g]] for g in ("f1", "g2", "f2", "g3")] + [offs[groups["zero"]] + 1] +
            [offs[d0 + FIRST_OF_WINDOW_14] + 60, offs[d0 + LAST_OF_RUN_14] + 60])


class Main:
    def __init__(self, path, unplaced=True):
        self.path = path
        self.recs, self.groups, self.offs = write_main(path, unplaced)
        self.stream = inflate(path)
        self.refs = ref.refs_of(self.stream)
        self.all = split_stream(self.stream)[3]
        self.lay = ixref.Layout(path)
        assert len(self.all) == len(self.recs) and len(self.lay.coff) > 600


@pytest.fixture(scope="module")
def main(tmp_path_factory):
    return Main(str(tmp_path_factory.mktemp("viewidx") / "main.bam"))


@pytest.fixture(scope="module")
def main_placed_only(tmp_path_factory):
    return Main(str(tmp_path_factory.mktemp("viewidx_p") / "placed.bam"), unplaced=False)


def run_case(m, tmp_path, tag, regions=(), bed_lines=None, keep=None, **opts):
    """count, BAM and SAM with use_index=True against the restatements, against OFF byte for byte, and blocks_read / runs against
    the .bai.  Returns (expected records, stats of the indexed BAM call)."""
    import sambamba_amd
    parsed = [ref.parse_region(r, m.refs) for r in regions]
    bed_merged = ref.merged_bed(bed_lines, m.refs) if bed_lines is not None else None
    sel = dict(keep=keep, regions=parsed or None, bed=bed_merged)
    if "num_filter" in opts:
        sel["bits"] = ref.num_filter(opts["num_filter"])
    if "subsample" in opts:
        sel["subsample"] = (opts["subsample"], opts["seed"])
    want = ref.select(m.all, **sel)
    bed = None
    if bed_lines is not None:
        bed = str(tmp_path / (tag + ".bed"))
        open(bed, "w").write("".join(l + "\n" for l in bed_lines))
    kw = dict(regions=regions, bed=bed, **opts)
    want_runs = ixref.runs_read(m.path, parsed if bed_merged is None else bed_merged)
    want_blocks = sum(b1 - b0 for b0, b1 in want_runs)

    def cost(st):
        print("%s: blocks_read %d of %d (reference %d), runs %d (reference %d), n_records_in %d of %d, n_batches %d" % (
            tag, st["blocks_read"], st["blocks_in_file"], want_blocks, st["runs"], len(want_runs), st["n_records_in"], len(m.all), st["n_batches"]))
        assert st["blocks_read"] == want_blocks and st["runs"] == len(want_runs)
        assert st["blocks_in_file"] == len(m.lay.coff)                          # (the blocks in front of the EOF block)
        assert st["blocks_read"] < st["blocks_in_file"] and st["n_records_in"] < len(m.all)
        assert st["inflated_bytes_read"] == sum(m.lay.off[b1] - m.lay.off[b0] for b0, b1 in want_runs)

    n_off = sambamba_amd.view(m.path, count=True, **kw)
    n_ix, st_c = sambamba_amd.view(m.path, count=True, use_index=True, with_stats=True, **kw)
    assert n_ix == n_off == len(want)
    cost(st_c)
    outs = {}
    for fmt in ("bam", "sam"):
        for mode in (False, True):
            out = str(tmp_path / ("%s.%s.%s" % (tag, "ix" if mode else "off", fmt)))
            extra = dict(command_line="view " + tag) if fmt == "bam" else dict(format="sam")
            outs[fmt, mode] = (out, sambamba_amd.view(m.path, out, use_index=mode, **extra, **kw))
        a, b = outs[fmt, False][0], outs[fmt, True][0]
        assert open(a, "rb").read() == open(b, "rb").read()
        st = outs[fmt, True][1]
        cost(st)
        assert st["n_entries_out"] == len(want) and st["n_records_in"] == st_c["n_records_in"]
        assert "blocks_read" not in outs[fmt, False][1]
    check_file(outs["bam", True][0], ref.expected_stream(m.stream, "view " + tag, **sel))
    assert open(outs["sam", True][0], "rb").read() == sam_ref.sam_text(want, [n for n, _ in m.refs])
    return want, outs["bam", True][1]


def names(recs):
    return [ref.fields(r)[4].decode() for r in recs]


@pytest.fixture
def batch_env(monkeypatch):
    def set_batch(batch):
        if batch is None:
            monkeypatch.delenv("SBX_INDEX_BATCH_BYTES", raising=False)
        else:
            monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    return set_batch


@BATCHES
def test_far_starting_and_zero_length_records(main, tmp_path, batch_env, batch):
    batch_env(batch)
    # the only record over chr1:1100005-1100015 starts a million positions in front of it and lies in a bin of 8 Mbp
    want, st = run_case(main, tmp_path, "far", ["chr1:1100005-1100015"])
    assert names(want) == ["far"] and st["n_records_in"] < 200
    # a record that covers no base is selected strictly inside a region, not at pos == start
    want, _ = run_case(main, tmp_path, "zero", ["chr1:400001-400100"])
    assert names(want) == ["far", "z_plain", "zero_inside"]


@BATCHES
def test_empty_selections(main, tmp_path, batch_env, batch):
    batch_env(batch)
    for tag, region in {"empty_window": "chr1:2500001-2500100", "empty_contig": "chr2:1-5000", "behind_the_last": "chr3:20001-20100"}.items():
        want, st = run_case(main, tmp_path, tag, [region])
        assert want == [] and st["runs"] == 0 and st["blocks_read"] == 0 and st["n_records_in"] == 0 and st["n_batches"] == 0
        # header + EOF
        assert st["stream_bytes"] == len(ref.expected_stream(main.stream, "view " + tag, regions=[ref.parse_region(region, main.refs)]))


@BATCHES
def test_run_boundaries(main, tmp_path, batch_env, batch):
    batch_env(batch)
    m = main
    d0 = m.groups["dense"]
    # the run of window 14 (229376 .. 245759): from the record that reaches into it first to the last record of the level-4 bin, which
    # crosses into window 15; both straddle a block boundary
    for k in (d0 + FIRST_OF_WINDOW_14, d0 + LAST_OF_RUN_14):
        assert m.offs[k] + 60 in m.lay.off
    want, st = run_case(m, tmp_path, "straddlers", ["chr1:229377-229400"])
    assert names(want) == ["far", "a0734"]
    # (what is read besides the run: `far`, and the records over 212992 and 262144, which lie in the 128 kbp and 1 Mbp bins of the region)
    assert st["n_records_in"] == LAST_OF_RUN_14 - FIRST_OF_WINDOW_14 + 1 + 3
    if batch:
        assert st["n_batches"] >= 3
    # a chunk that begins at the last byte of a block: the window of `zero` starts with a record one byte in front of a boundary
    z = m.groups["zero"]
    assert m.offs[z] + 1 in m.lay.off
    want, st = run_case(m, tmp_path, "last_byte", ["chr1:400001-400060"])
    assert names(want) == ["far", "z_plain", "zero_inside"]
    # runs one block apart are joined, runs three blocks apart are not
    gap = lambda a, b: m.lay.block_of(m.offs[m.groups[b]]) - m.lay.block_of(m.offs[m.groups[a]] - 1) - 1
    assert gap("f1", "g2") == 1 and gap("f2", "g3") == 3
    want, st = run_case(m, tmp_path, "one_apart", ["chr1:1190001-1190200", "chr1:1230001-1230200"])
    assert st["runs"] == 1 and len(want) == 24 and st["n_records_in"] == 28             # (the four records between them are read)
    want, st = run_case(m, tmp_path, "three_apart", ["chr1:1230001-1230200", "chr1:1270001-1270200"])
    assert st["runs"] == 2 and len(want) == 24 and st["n_records_in"] == 24


@BATCHES
def test_overlapping_regions_bed_and_star(main, main_placed_only, tmp_path, batch_env, batch):
    batch_env(batch)
    # listed regions that overlap: duplicates, in listed order
    regions = ["chr1:210001-215000", "chr3:1-2000", "chr1:205001-212000"]
    want, st = run_case(main, tmp_path, "overlapping", regions)
    assert len(set(names(want))) < len(want) and names(want).count("far") == 2 and st["n_regions"] == 3
    # a BED file of 300 intervals, merged
    bed = ["chr1\t%d\t%d" % (200000 + 390 * k, 200000 + 390 * k + 120) for k in range(298)][::-1] + ["chr3\t500\t900", "chrUn\t5\t10"]
    want, st = run_case(main, tmp_path, "bed300", bed_lines=bed)
    assert len(want) > 500
    if batch:
        assert st["n_batches"] >= 3
    # `*`: alone, between two regions, and on a file without unplaced reads
    want, st = run_case(main, tmp_path, "star", ["*"])
    assert len(want) == 40 and st["runs"] == 1 and st["n_records_in"] == 40
    want, _ = run_case(main, tmp_path, "star_between", ["chr3:1-500", "*", "chr1:400001-400100"])
    assert names(want)[-3:] == ["far", "z_plain", "zero_inside"] and names(want).count("u00") == 1
    want, st = run_case(main_placed_only, tmp_path, "star_none", ["*"])
    assert want == [] and st["runs"] == 0
    want, _ = run_case(main_placed_only, tmp_path, "star_none_with_region", ["*", "chr3:1-500"])
    assert len(want) > 5


def test_options_combined(main, tmp_path, monkeypatch):
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", SMALL_BATCH)

    def keep(r):
        return ref.fields(r)[3] >= 30
    want, st = run_case(main, tmp_path, "combined", ["chr1:230001-290000", "*"], keep=keep, filter="mapping_quality >= 30",
                        num_filter="/4", subsample=0.5, seed=12345, valid=True)
    assert 100 < len(want) < 1000 and st["n_batches"] >= 3


def test_cost_follows_the_region(main, tmp_path):
    """blocks_read is the reference's figure exactly (run_case); and for a region over hundreds of blocks it is at most the blocks that
    hold the records that overlap the region plus those of the records of the two 16 kbp edge windows."""
    m = main
    beg, end = 203000, 315000
    want, st = run_case(m, tmp_path, "cost", ["chr1:%d-%d" % (beg + 1, end)])
    d0 = m.groups["dense"]
    pos = lambda k: 200000 + 40 * (k - d0)
    blocks_of = lambda ks: {b for k in ks for b in range(m.lay.block_of(m.offs[k]), m.lay.block_of(m.offs[k + 1] - 1) + 1)}
    inside = blocks_of([m.groups["far"]] + [k for k in range(d0, d0 + 3000) if pos(k) < end and pos(k) + 50 > beg])
    lo, hi = (beg >> 14) << 14, ((end >> 14) + 1) << 14
    edges = blocks_of(k for k in range(d0, d0 + 3000) if (lo < pos(k) + 50 and pos(k) < beg) or (end <= pos(k) < hi))
    print("cost: blocks_read %d, inside %d, edge windows %d, file %d" % (st["blocks_read"], len(inside), len(edges - inside), st["blocks_in_file"]))
    assert len(inside) > 500
    assert st["blocks_read"] <= len(inside | edges)
    assert st["n_records_in"] < len(m.all)


# ---- failures ----
def refused(code, word, out, *args, **kw):
    import sambamba_amd
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(*args, **kw)
    assert ei.value.code == code and word in str(ei.value), str(ei.value)
    assert out is None or not os.path.exists(out)


def test_failures_leave_no_output(main, tmp_path, monkeypatch):
    import sambamba_amd
    m = main
    out = str(tmp_path / "refused.out")
    sinks = [dict(count=True), dict(out_path=out), dict(out_path=out, format="sam")]
    # no .bai: REQUIRED refuses, AUTO is OFF
    bare = str(tmp_path / "bare.bam")
    shutil.copy(m.path, bare)
    for sink in sinks:
        refused(-7, ".bai", out, bare, regions=["chr1:400001-400100"], use_index=True, **sink)
    assert sambamba_amd.view(bare, count=True, regions=["chr1:400001-400100"], use_index="auto") == 3
    assert sambamba_amd.view(bare, count=True, use_index=True) == len(m.all)               # nothing to restrict: no index needed
    a, b = str(tmp_path / "auto.bam"), str(tmp_path / "off.bam")
    st = sambamba_amd.view(bare, a, regions=["chr1:400001-400100"], use_index="auto", command_line="x")
    sambamba_amd.view(bare, b, regions=["chr1:400001-400100"], command_line="x")
    assert open(a, "rb").read() == open(b, "rb").read()
    assert st["blocks_read"] == st["blocks_in_file"] and st["n_records_in"] == len(m.all)
    # without a region every mode is OFF
    n, st = sambamba_amd.view(m.path, count=True, use_index=True, with_stats=True)
    assert n == len(m.all) and st["blocks_read"] == st["blocks_in_file"] and st["n_records_in"] == len(m.all)
    # the .bai of a file with another number of references
    other = str(tmp_path / "other.bam")
    write(other, [rec(0, 100 + k, "20M", "o%02d" % k) for k in range(20)], refs=REFS[:2])
    foreign = str(tmp_path / "foreign.bam")
    shutil.copy(m.path, foreign)
    shutil.copy(other + ".bai", foreign + ".bai")
    for sink in sinks:
        refused(-3, "", out, foreign, regions=["chr1:1-1000"], use_index=True, **sink)
    # the .bai of the sorted file next to a copy with two records of one queried run swapped
    recs = list(m.recs)
    i, j = m.groups["dense"] + 1000, m.groups["dense"] + 1003
    assert len(recs[i]) == len(recs[j])
    recs[i], recs[j] = recs[j], recs[i]
    swapped = str(tmp_path / "swapped.bam")
    bamgen.write_bam(swapped, REFS, recs, block_size=BLOCK, cuts=main_cuts(m.groups, m.offs), write_index=False)
    shutil.copy(m.path + ".bai", swapped + ".bai")
    for sink in sinks:
        refused(-6, "order", out, swapped, regions=["chr1:239001-241000"], use_index=True, **sink)
    # ... also when the pair lies in a later piece of a run that is cut
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", SMALL_BATCH)
    refused(-6, "order", out, swapped, regions=["chr1:239001-241000"], use_index=True, out_path=out)
    monkeypatch.delenv("SBX_INDEX_BATCH_BYTES")
    # (a run that does not hold the pair reads fine)
    assert sambamba_amd.view(swapped, count=True, regions=["chr1:400001-400100"], use_index=True) == 3
    # an unknown reference and an empty region, as without the index
    for sink in sinks:
        refused(-1, "chrNope", out, m.path, regions=["chr1:1-10", "chrNope:5-9"], use_index=True, **sink)
        refused(-1, "empty", out, m.path, regions=["chr1:300-200"], use_index=True, **sink)
    with pytest.raises(ValueError):
        sambamba_amd.view(m.path, count=True, use_index="yes")


# ---- sbx-iview ----
def iview(args, env=None):
    from sambamba_amd import iview_cli_path
    return subprocess.run([iview_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def test_iview_cli(main, tmp_path):
    m = main
    regions = ["chr1:230001-232000", "chr3:1-300", "*"]
    parsed = [ref.parse_region(r, m.refs) for r in regions]
    want = ref.select(m.all, regions=parsed)
    r = iview([])
    assert r.returncode == 0 and r.stderr.startswith(b"Usage: sbx-iview [options] <input.bam> [region1 [...]]\n") and b"--no-index" in r.stderr
    # -c, with the timing line
    r = iview(["-c", m.path] + regions, env={"SBX_TIMING": "1"})
    assert r.returncode == 0 and r.stdout == b"%d\n" % len(want), r.stderr
    line = [l for l in r.stderr.decode().splitlines() if l.startswith("[sbx] view-index:")]
    assert len(line) == 1
    figures = dict(f.split("=") for f in line[0].split()[2:])
    assert set(figures) == {"blocks_in_file", "blocks_read", "runs", "compressed_bytes_read", "inflated_bytes_read", "ms_plan"}
    assert int(figures["blocks_read"]) == len(ixref.blocks_read(m.path, parsed)) < int(figures["blocks_in_file"])
    r = iview(["-c", "--no-index", m.path] + regions, env={"SBX_TIMING": "1"})
    assert r.returncode == 0 and r.stdout == b"%d\n" % len(want) and b"view-index" not in r.stderr
    # SAM (the default) and BAM, to stdout: the same bytes with and without the index (--no-index is not part of the @PG line)
    for fmt_args, tag in (([], "sam"), (["-h"], "samh"), (["-f", "bam"], "bam")):
        a = iview(fmt_args + [m.path] + regions)
        b = iview(fmt_args + ["--no-index", m.path] + regions)
        assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
        assert a.stdout == b.stdout and len(a.stdout) > 1000
        if tag == "sam":
            assert a.stdout == sam_ref.sam_text(want, [n for n, _ in m.refs])
        if tag == "bam":
            out = str(tmp_path / "stdout.bam")
            open(out, "wb").write(a.stdout)
            check_file(out, ref.expected_stream(m.stream, "view " + " ".join(fmt_args + [m.path] + regions), regions=parsed))
    # -L, and the refusal without a .bai
    bed = str(tmp_path / "r.bed")
    open(bed, "w").write("chr1\t230000\t232000\nchr3\t0\t300\n")
    r = iview(["-c", "-L", bed, m.path])
    assert r.returncode == 0 and int(r.stdout) == len(ref.select(m.all, bed=ref.merged_bed(open(bed).read().splitlines(), m.refs)))
    bare = str(tmp_path / "bare.bam")
    shutil.copy(m.path, bare)
    out = str(tmp_path / "bare.out.bam")
    r = iview(["-f", "bam", "-o", out, bare, "chr1:1-1000"])
    assert r.returncode == 1 and r.stderr.startswith(b"sbx-iview: ") and b".bai" in r.stderr and not os.path.exists(out)
    r = iview(["-c", "--no-index", bare, "chr1:400001-400100"])
    assert r.returncode == 0 and r.stdout == b"3\n"
    r = iview(["-c", bare])
    assert r.returncode == 0 and int(r.stdout) == len(m.all)


def test_abi_size():
    import ctypes as C
    from sambamba_amd import _lib
    L = _lib.lib()
    assert L.sbx_abi_sizeof(b"sbx_view_index_stats") == C.sizeof(_lib.ViewIndexStats) == 48
    assert L.sbx_abi_sizeof(b"sbx_view_request") == 96
