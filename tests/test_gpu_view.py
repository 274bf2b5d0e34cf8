"""`sambamba view` on the device -- sbx_view_count / sbx_view_bam: K12a selection and K12b emission (view.hip) between the read pass
and the writer of sort -- through the Python API and the `sbx-view` CLI, against the pure-Python restatement of view.d
(tests/view_ref.py) applied to the inflated input.  Every BAM is compared byte for byte on its INFLATED stream -- header with the @PG
line, then the records in the expected order --; the file itself must scan as BGZF, end with the EOF block and hold no block of more
than 0xFF00 payload bytes."""
import collections
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import view_ref as ref
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream
from tests.test_gpu_sort import REFS, UNSORTED, _tie_records, check_file
from tests.util import GOLDEN, gen_bam, scan_bgzf

pytestmark = pytest.mark.gpu

FIXTURES = ("issue225", "issue_193", "issue_204", "mate_overlaps_1_3M_4M", "match_mates")
REF_LIST = [(n, l) for n, l in REFS]


def cli(args, env=None):
    from sambamba_amd import view_cli_path
    return subprocess.run([view_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def _keep_q30_not_dup(rec):
    bin_mq_nl, flag_nc = struct.unpack_from("<II", rec, 12)
    return ((bin_mq_nl >> 8) & 0xFF) >= 30 and not (flag_nc >> 16) & 0x400


def check(path, tmp_path, tag="o", flt=None, keep=None, num_filter=None, regions=(), bed_lines=None, subsample=None, seed=None, level=-1, env=None):
    """count and BAM through the API and the CLI against the restatement; returns (expected records, API stats)."""
    import sambamba_amd
    stream = inflate(path)
    refs = ref.refs_of(stream)
    sel = dict(keep=keep,
               bits=ref.num_filter(num_filter) if num_filter is not None else None,
               subsample=(subsample, seed) if subsample is not None else None,
               regions=[ref.parse_region(r, refs) for r in regions] or None,
               bed=ref.merged_bed(bed_lines, refs) if bed_lines is not None else None)
    want_recs = ref.select(split_stream(stream)[3], **sel)
    bed = None
    if bed_lines is not None:
        bed = str(tmp_path / (tag + ".bed"))
        open(bed, "w").write("".join(l + "\n" for l in bed_lines))
    kw = dict(filter=flt, num_filter=num_filter, regions=regions, bed=bed, subsample=subsample, seed=seed)
    # ---- API
    n = sambamba_amd.view(path, count=True, **kw)
    print("%s: count %d, expected %d" % (tag, n, len(want_recs)))
    assert n == len(want_recs)
    out_api = str(tmp_path / (tag + ".api.bam"))
    st = sambamba_amd.view(path, out_api, level=level, command_line="view " + tag, **kw)
    check_file(out_api, ref.expected_stream(stream, "view " + tag, **sel))
    assert not os.path.exists(out_api + ".bai")
    assert st["n_entries_out"] == len(want_recs) and st["n_records_in"] == len(split_stream(stream)[3])
    assert st["compressed_bytes"] == os.path.getsize(out_api)
    # ---- CLI
    args = []
    if flt:
        args += ["-F", flt]
    if num_filter is not None:
        args += ["--num-filter=" + num_filter]
    if subsample is not None:
        args += ["-s", repr(subsample), "--subsampling-seed", str(seed)]
    if bed:
        args += ["-L", bed]
    if level != -1:
        args += ["-l", str(level)]
    r = cli(["-c"] + args + [path] + list(regions), env=env)
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"%d\n" % len(want_recs)
    out_cli = str(tmp_path / (tag + ".cli.bam"))
    full = ["-f", "bam", "-o", out_cli] + args + [path] + list(regions)
    r = cli(full, env=env)
    assert r.returncode == 0 and r.stdout == b"", r.stderr
    check_file(out_cli, ref.expected_stream(stream, "view " + " ".join(full), **sel))
    assert not os.path.exists(out_cli + ".bai")
    return want_recs, st


# ---- goldens ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_fixtures(name, tmp_path):
    path = os.path.join(GOLDEN, name + ".bam")
    n_all = len(split_stream(inflate(path))[3])
    want, st = check(path, tmp_path)
    assert len(want) == n_all == st["n_records_selected"]
    want, _ = check(path, tmp_path, tag="f", flt="mapping_quality >= 30 and not duplicate", keep=_keep_q30_not_dup)
    assert len(want) <= n_all


# ---- region edges -----------------------------------------------------------------------------------------------------------------
START, END = 100, 110          # "c1:101-110"
CIGARS = {0: [""], 1: ["2S1M", "1M3I", "1M5H"], 2: ["1M1D", "1M1N", "1S2M1S", "1=1X"]}


def _qlen(cigar):
    return sum(n for op, n in bamgen.parse_cigar(cigar) if op in "MIS=X")


def _edge_records():
    recs, k = [], 0
    for pos in (START - 2, START - 1, START, START + 1, END - 1, END):
        for cov, cigars in CIGARS.items():
            for cg in cigars:
                for r in (0, 1):                                   # the region's reference and the wrong one
                    seq = "ACGTACGT"[:_qlen(cg)] if cg else "ACG"
                    recs.append(bamgen.make_record(r, pos, cg, seq, 30, name="e%03d_p%d_c%d_%s" % (k, pos, cov, cg or "none")))
                    k += 1
    # flagged unmapped but placed: covers nothing whatever its CIGAR says
    for pos in (START - 1, START, START + 1, END - 1):
        recs.append(bamgen.make_record(0, pos, "5M", "ACGTA", 30, name="u%03d_p%d" % (k, pos), flag=0x4, mapq=0))
        k += 1
    # no reference
    for pos in (-1, START + 1):
        recs.append(bamgen.make_record(-1, pos, "", "ACGT", 30, name="n%03d" % k, flag=0x4, mapq=0))
        k += 1
    # a long alignment that starts far in front of the region and one that ends exactly at its start
    recs.append(bamgen.make_record(0, 10, "20M70N10M", "A" * 30, 30, name="long%03d" % k))
    recs.append(bamgen.make_record(0, 10, "20M60N10M", "A" * 30, 30, name="touch%03d" % (k + 1)))
    return recs


@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("viewedges") / "edges.bam")
    bamgen.write_bam(path, REFS, _edge_records(), text=UNSORTED, write_index=False)
    return path


def test_region_edges(edges, tmp_path):
    want, _ = check(edges, tmp_path, regions=["c1:%d-%d" % (START + 1, END)])
    names = [ref.fields(r)[4].decode() for r in want]
    # the table of tests/test_view_core_cpu.py, on records: by position and bases covered, whatever the CIGAR that covers them
    by = {}
    for nm in names:
        if nm.startswith("e"):
            _, p, c, _ = nm.split("_", 3)
            by.setdefault((int(p[1:]), int(c[1:])), 0)
            by[(int(p[1:]), int(c[1:]))] += 1
    n_cig = {c: len(v) for c, v in CIGARS.items()}
    assert by == {(START - 1, 2): n_cig[2], (START, 1): n_cig[1], (START, 2): n_cig[2], (START + 1, 0): n_cig[0], (START + 1, 1): n_cig[1],
                  (START + 1, 2): n_cig[2], (END - 1, 0): n_cig[0], (END - 1, 1): n_cig[1], (END - 1, 2): n_cig[2]}
    placed = sorted(int(nm.split("_p")[1]) for nm in names if nm.startswith("u"))
    assert placed == [START + 1, END - 1]                     # an unmapped read at pos == start is not selected, inside it is
    assert sum(nm.startswith("long") for nm in names) == 1 and not any(nm.startswith("touch") for nm in names)
    want, _ = check(edges, tmp_path, tag="star", regions=["*"])
    assert len(want) == 2 and all(ref.fields(r)[0] == -1 for r in want)
    check(edges, tmp_path, tag="mix", regions=["c1:%d-%d" % (START + 1, END), "*", "c2", "c1"])


def test_many_listed_regions_and_the_cap(edges, tmp_path):
    import sambamba_amd
    regions = ["c1:%d-%d" % (k + 1, k + 10) for k in range(1023)] + ["*"]
    want, st = check(edges, tmp_path, regions=regions)
    assert st["n_regions"] == 1024 and len(want) > st["n_records_selected"] > 0       # records come out several times
    for count in (True, False):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.view(edges, str(tmp_path / "cap.bam"), count=count, regions=regions + ["c2"])
        assert ei.value.code == -1 and "1024" in ei.value.msg
    assert not os.path.exists(str(tmp_path / "cap.bam"))


# ---- listed regions that overlap one another, BED ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ties(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("viewties") / "ties.bam")
    bamgen.write_bam(path, REFS, _tie_records(n=3000, seed=31), text=UNSORTED, write_index=False)
    return path


LISTED = ["c1:1-200", "c1:50-150", "c2", "c1:1-200", "*", "c2:5000-5000"]


def test_overlapping_listed_regions(ties, tmp_path):
    fwd, st = check(ties, tmp_path, regions=LISTED)
    assert st["n_entries_out"] > st["n_records_selected"] and st["n_sort_passes"] >= 1
    rev, _ = check(ties, tmp_path, tag="rev", regions=LISTED[::-1])
    assert sorted(fwd) == sorted(rev) and fwd != rev
    # a record of both c1 regions is there three times (c1:1-200 is listed twice)
    n_rec = len(split_stream(inflate(ties))[3])
    assert max(collections.Counter(fwd).values()) == 3 and len(fwd) > n_rec // 2


def test_bed_selects_once_in_file_order(ties, tmp_path):
    lines = ["c1\t49\t150", "c2\t0\t50000", "c1\t0\t200\tname", "chrNotThere\t0\t10", "c1\t0\t200", "c2\t4999\t5000", "c1 4999"]
    want, st = check(ties, tmp_path, bed_lines=lines)
    assert len(set(want)) == len(want) == st["n_records_selected"] > 0
    recs = split_stream(inflate(ties))[3]
    order = {r: k for k, r in enumerate(recs)}
    assert [order[r] for r in want] == sorted(order[r] for r in want)
    want, _ = check(ties, tmp_path, tag="none", bed_lines=["chrNotThere\t0\t10"])
    assert want == []


def test_golden_bed(tmp_path):
    path = os.path.join(GOLDEN, "mate_overlaps_1_3M_4M.bam")
    lines = open(os.path.join(GOLDEN, "mate_overlaps_1_3M_4M.bed")).read().splitlines()
    want, _ = check(path, tmp_path, bed_lines=lines)
    assert len(want) > 0


# ---- subsampling, --num-filter ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("viewpairs") / "pairs.bam")
    recs = []
    for k in range(700):
        name = "pair%04d" % k if k % 7 else "q" * (1 + k % 254)
        recs.append(bamgen.make_record(k % 2, 100 + 3 * k, "10M", "ACGTACGTAC", 30, name=name, flag=0x43, next_ref=k % 2, next_pos=300 + 3 * k))
        recs.append(bamgen.make_record(k % 2, 300 + 3 * k, "10M", "ACGTACGTAC", 30, name=name, flag=0x93, next_ref=k % 2, next_pos=100 + 3 * k))
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, write_index=False)
    return path


@pytest.mark.parametrize("seed", [0, 2 ** 63 + 5])
@pytest.mark.parametrize("fraction", [0.0, 0.25, 1.0])
def test_subsample(pairs, tmp_path, seed, fraction):
    want, _ = check(pairs, tmp_path, subsample=fraction, seed=seed)
    names = [ref.fields(r)[4] for r in want]
    n_all = len(split_stream(inflate(pairs))[3])
    if fraction == 0.0:
        assert names == []
    elif fraction == 1.0:
        assert len(names) == n_all
    else:
        assert 0 < len(names) < n_all
    assert all(v % 2 == 0 for v in collections.Counter(names).values())                 # both mates of a pair share the verdict


@pytest.mark.parametrize("num_filter", ["4/", "/4", "3/1024"])
def test_num_filter(ties, pairs, tmp_path, num_filter):
    path = pairs if num_filter.startswith("3") else ties
    want, _ = check(path, tmp_path, num_filter=num_filter)
    assert 0 < len(want) <= len(split_stream(inflate(path))[3])
    # with -F, a region and -s in one call
    check(ties, tmp_path, tag="all", num_filter=num_filter.replace("3/", "16/"), flt="mapping_quality >= 30 and not duplicate",
          keep=_keep_q30_not_dup, regions=["c1:1-5000", "c2"], subsample=0.5, seed=7)


# ---- layouts and batches ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    d = tmp_path_factory.mktemp("viewlayouts")
    recs = _tie_records(n=4000, seed=11)
    long_seq = "ACGT" * 300                                   # a record larger than a 300- or 1000-byte block
    for k in (10, 2000, 3999):
        recs.insert(k, bamgen.make_record(0, 100, "1200M", long_seq, 30, name="long%04d" % k))
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
    return files, info


SELECTION = dict(flt="mapping_quality >= 30 and not duplicate", keep=_keep_q30_not_dup, regions=["c1:1-200", "c2", "c1:100-101", "*"])


@pytest.mark.parametrize("kind", ["all", "cuts", "tiny", "levels"])
def test_layouts_and_batches(layouts, kind, tmp_path, monkeypatch):
    import sambamba_amd
    files, info = layouts
    path = files[kind]
    one, st = check(path, tmp_path, **SELECTION)
    assert st["n_batches"] == 1 and len(one) > 0
    batch = str(min(info["stream_len"] // 5, 60000))
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    many, st = check(path, tmp_path, tag="b", env={"SBX_INDEX_BATCH_BYTES": batch}, **SELECTION)
    assert st["n_batches"] >= 3
    assert many == one
    a, b = inflate(str(tmp_path / "o.api.bam")), inflate(str(tmp_path / "b.api.bam"))
    assert split_stream(a)[3] == split_stream(b)[3]
    # BED and no region at all in batches
    check(path, tmp_path, tag="bb", env={"SBX_INDEX_BATCH_BYTES": batch}, bed_lines=["c1\t0\t150", "c2\t4000\t6000"], num_filter="/16")
    check(path, tmp_path, tag="bn", env={"SBX_INDEX_BATCH_BYTES": batch}, flt="reverse_strand",
          keep=lambda r: bool((struct.unpack_from("<I", r, 16)[0] >> 16) & 0x10))
    r = cli(["-c", path], env={"SBX_INDEX_BATCH_BYTES": batch, "SBX_TIMING": "1"})
    line = [x for x in r.stderr.decode().splitlines() if x.startswith("[sbx] view:")]
    assert len(line) == 1 and "sink=count" in line[0] and "ms_select=" in line[0]


# ---- empty outputs, output options ----------------------------------------------------------------------------------------------------
def test_empty_selection_and_header_only_input(ties, tmp_path):
    import sambamba_amd
    want, st = check(ties, tmp_path, flt="mapping_quality > 254", keep=lambda r: False)
    assert want == [] and st["n_entries_out"] == 0
    got = inflate(str(tmp_path / "o.api.bam"))
    assert split_stream(got)[3] == [] and b"@PG\tID:sambamba\tCL:view o" in got
    empty = str(tmp_path / "empty.bam")
    bamgen.write_bam(empty, REFS, [], text=UNSORTED, write_index=False)
    want, st = check(empty, tmp_path, tag="e")
    assert want == [] and st["n_records_in"] == 0
    check(empty, tmp_path, tag="er", regions=["c1", "*"])
    assert sambamba_amd.view(empty, count=True, bed=None, regions=["c2:1-10"]) == 0


def test_levels_inflate_to_the_same_stream(ties, tmp_path):
    sizes = {}
    for level in (0, 1, 6):
        check(ties, tmp_path, tag="l%d" % level, level=level, regions=["c1", "c2:1-20000"])
        sizes[level] = os.path.getsize(str(tmp_path / ("l%d.api.bam" % level)))
    assert sizes[0] > sizes[1] >= sizes[6]


def test_index_of_a_bed_selection(tmp_path):
    import sambamba_amd
    from tests.test_bai_cpu import SRC, parse_bai
    bam = gen_bam(str(tmp_path / "s.bam"), "chrA:60000,chrB:30000", coverage=6, seed=3)
    bed = str(tmp_path / "s.bed")
    open(bed, "w").write("chrA\t1000\t20000\nchrB\t500\t25000\nchrA\t40000\t41000\n")
    out = str(tmp_path / "sel.bam")
    st = sambamba_amd.view(bam, out, bed=bed, index=True)
    stream = inflate(bam)
    lines = open(bed).read().splitlines()
    check_file(out, ref.expected_stream(stream, None, bed=ref.merged_bed(lines, ref.refs_of(stream))))
    assert 0 < st["n_entries_out"] < st["n_records_in"] and os.path.exists(out + ".bai")
    exe = str(tmp_path / "bai_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", "-o", exe, SRC, "-lz"])
    cpu = str(tmp_path / "cpu.bai")
    subprocess.check_call([exe, out, cpu])
    mine, tail_m = parse_bai(out + ".bai")
    want, tail_w = parse_bai(cpu)
    assert tail_m == tail_w and len(mine) == len(want) == 2
    for (bm, lm, _), (bw, lw, _) in zip(mine, want):
        assert bm == bw and lm == lw
    assert sum(len(b) for b, _, _ in mine) > 0


# ---- failures -------------------------------------------------------------------------------------------------------------------------
def _codes(path, tmp_path):
    """(code of sbx_sort_bam, code of sbx_view_bam, code of sbx_view_count); no output file is left."""
    import sambamba_amd
    codes = []
    for call in (lambda o: sambamba_amd.sort_bam(path, o), lambda o: sambamba_amd.view(path, o), lambda o: sambamba_amd.view(path, count=True)):
        out = str(tmp_path / "fail.bam")
        with pytest.raises(sambamba_amd.SbxError) as ei:
            call(out)
        codes.append(ei.value.code)
        assert not os.path.exists(out) and not os.path.exists(out + ".bai")
    out = str(tmp_path / "failcli.bam")
    r = cli(["-f", "bam", "-o", out, path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"sbx-view: ")
    assert not os.path.exists(out)
    r = cli(["-c", path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"sbx-view: ")
    return codes


def test_missing_truncated_and_corrupt(layouts, tmp_path):
    files, info = layouts
    assert _codes(str(tmp_path / "no_such.bam"), tmp_path) == [-2, -2, -2]
    raw = open(files["all"], "rb").read()
    cut = str(tmp_path / "cut.bam")
    open(cut, "wb").write(raw[:len(raw) // 2])
    s, v, c = _codes(cut, tmp_path)
    assert s == v == c == -3
    bad = str(tmp_path / "bad.bam")
    _, co, _, _, _, _ = scan_bgzf(files["levels"])
    b = bytearray(open(files["levels"], "rb").read())
    b[int(co[len(co) // 2])] = 0xFF
    open(bad, "wb").write(b)
    s, v, c = _codes(bad, tmp_path)
    assert s == v == c == -3
    badref = str(tmp_path / "badref.bam")
    recs = [bamgen.make_record(0, 10, "4M", "ACGT", 30, name="a"), bamgen.make_record(2, 10, "4M", "ACGT", 30, name="b")]
    bamgen.write_bam(badref, REFS, recs, text=UNSORTED, write_index=False)
    s, v, c = _codes(badref, tmp_path)
    assert s == v == c == -3


def test_output_must_not_be_the_input_and_unknown_reference(ties, tmp_path):
    import sambamba_amd
    path = str(tmp_path / "in.bam")
    bamgen.write_bam(path, REFS, _tie_records(n=50), text=UNSORTED, write_index=False)
    before = open(path, "rb").read()
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(path, path)
    assert ei.value.code == -1
    r = cli(["-f", "bam", "-o", str(tmp_path / "." / "in.bam"), path])
    assert r.returncode == 1 and r.stderr.startswith(b"sbx-view: the output would overwrite the input")
    assert open(path, "rb").read() == before
    out = str(tmp_path / "x.bam")
    for count in (True, False):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.view(ties, out, count=count, regions=["c1", "chrNotThere:1-10"])
        assert ei.value.code == -1 and "chrNotThere" in ei.value.msg
    r = cli(["-f", "bam", "-o", out, ties, "chrNotThere"])
    assert r.returncode == 1 and b"chrNotThere" in r.stderr and not os.path.exists(out)
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(ties, count=True, bed=str(tmp_path / "no_such.bed"))
    assert ei.value.code == -2
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(ties, count=True, regions=["c1"], bed=str(tmp_path / "no_such.bed"))
    assert ei.value.code == -1 and "disallowed" in ei.value.msg
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(ties, count=True, subsample=-0.5, seed=1)
    assert ei.value.code == -1


# ---- interface ------------------------------------------------------------------------------------------------------------------------
def test_header_reference_info_and_precedence(ties, tmp_path):
    import sambamba_amd
    from tests.markdup_ref import header_text
    n = len(split_stream(inflate(ties))[3])
    r = cli(["-H", ties])
    assert (r.returncode, r.stdout) == (0, header_text(UNSORTED, None).encode()), r.stderr
    assert b"@PG" not in r.stdout
    r = cli(["-H", "-f", "bam", ties])
    assert (r.returncode, r.stdout) == (0, header_text(UNSORTED, None).encode())
    want = '["{name":"c1","length":100000},"{name":"c2","length":50000}]\n'
    assert want == ref.reference_info_json(REF_LIST)
    r = cli(["-I", ties])
    assert (r.returncode, r.stdout) == (0, want.encode()), r.stderr
    r = cli(["-I", "-H", ties])                                   # -I wins over -H
    assert (r.returncode, r.stdout) == (0, want.encode())
    assert sambamba_amd.view_reference_info(ties) == want
    for extra in (["-I"], ["-H"], ["-I", "-H", "-h", "-f", "json"]):                # -c wins over both
        r = cli(["-c"] + extra + [ties])
        assert (r.returncode, r.stdout) == (0, b"%d\n" % n), r.stderr


def test_bam_on_stdout(ties, tmp_path):
    stream = inflate(ties)
    for args in (["-f", "bam", "-o", "-", ties, "c2"], ["-f", "bam", ties, "c2"]):
        r = cli(args)
        assert r.returncode == 0, r.stderr
        out = str(tmp_path / "stdout.bam")
        open(out, "wb").write(r.stdout)
        check_file(out, ref.expected_stream(stream, "view " + " ".join(args), regions=[ref.parse_region("c2", REF_LIST)]))
    # a failure leaves stdout empty
    r = cli(["-f", "bam", ties, "chrNotThere"])
    assert r.returncode == 1 and r.stdout == b""


def test_abi_sizeof_view_structs():
    import sambamba_amd
    from sambamba_amd._lib import ViewOpts, ViewStats
    L = sambamba_amd.lib()
    assert L.sbx_abi_sizeof(b"sbx_view_opts") == C.sizeof(ViewOpts) == 24
    assert L.sbx_abi_sizeof(b"sbx_view_stats") == C.sizeof(ViewStats) == 6 * 8 + 4 * 4 + 8 * 8
