"""`sambamba view` with SAM output on the device -- sbx_view_sam: K13a / K13b (sam.hip, sam_core.hpp) behind the selection of
sbx_view_bam -- through the Python API and the `sbx-sam` CLI.  The whole output is compared byte for byte with the Python restatement
of the line (tests/sam_ref.py) applied to the entries tests/view_ref.py selects, and, independently of that restatement, with the
record lines of two SAM files of the reference's test data."""
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests import sam_cases as cases
from tests import sam_ref
from tests import view_ref as ref
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream
from tests.test_gpu_sort import REFS as TIE_REFS, UNSORTED, _tie_records
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu


def cli(args, env=None, exe=None):
    from sambamba_amd import sam_cli_path
    return subprocess.run([exe or sam_cli_path()] + list(args), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=dict(os.environ, **env) if env else None)


def expected_text(path, keep=None, num_filter=None, regions=(), bed_lines=None, subsample=None, seed=None):
    stream = inflate(path)
    refs = ref.refs_of(stream)
    sel = dict(keep=keep, bits=ref.num_filter(num_filter) if num_filter is not None else None,
               subsample=(subsample, seed) if subsample is not None else None,
               regions=[ref.parse_region(r, refs) for r in regions] or None,
               bed=ref.merged_bed(bed_lines, refs) if bed_lines is not None else None)
    recs = ref.select(split_stream(stream)[3], **sel)
    return sam_ref.sam_text(recs, [n for n, _ in refs]), len(recs)


def view_sam(path, tmp_path, tag="o", **kw):
    """the text and the stats of sambamba_amd.view(format="sam")"""
    import sambamba_amd
    out = str(tmp_path / (tag + ".sam"))
    st = sambamba_amd.view(path, out, format="sam", **kw)
    return open(out, "rb").read(), st


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(got), len(want), k, got[max(0, k - 40):k + 40], want[max(0, k - 40):k + 40])


# ---- every field and every tag type at its edges ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("samedges") / "edges.bam")
    bamgen.write_bam(path, cases.REFS, cases.edge_records() + cases.tag_records(), text=cases.TEXT, write_index=False)
    return path, expected_text(path)[0]


def test_edge_case_records_and_tags(edges, tmp_path):
    path, want = edges
    got, st = view_sam(path, tmp_path)
    assert got == want, first_difference(got, want)
    n = len(cases.edge_records() + cases.tag_records())
    assert st["n_entries_out"] == st["n_records_selected"] == st["n_records_in"] == n
    assert st["stream_bytes"] == len(want) and st["compressed_bytes"] == 0 and st["ms_deflate"] == 0
    # a few lines written out, so that the restatement is not the only witness
    by_name = {l.split(b"\t")[0]: l for l in got.split(b"\n")}
    assert by_name[b"pos2"] == b"pos2\t4\t*\t-2147483648\t0\t*\t*\t-2147483648\t2147483647\tAG\t??"
    assert by_name[b"cigops"].split(b"\t")[5] == b"1M2I3D4N5S6H7P8=9X10?11?12?13?14?15?16?"
    assert by_name[b"cigmax"].split(b"\t")[5].count(b"M") == 7282 and len(by_name[b"cigmax"]) > 250000
    floats = by_name[b"floats"].split(b"\t")[11:]
    assert floats[:9] == [b"f0:f:0", b"f1:f:-0", b"f2:f:1e-05", b"f3:f:123456", b"f4:f:1.23457e+06", b"f5:f:3.40282e+38", b"f6:f:1.4013e-45",
                          b"f7:f:inf", b"f8:f:nan"]
    assert floats[-1].startswith(b"Bf:B:f,-nan,nan,1.4013e-45,")
    assert b"\tA0:B:c,\t" in by_name[b"arrays"] and b"\tG0:B:f,\t" in by_name[b"arrays"]        # count 0: the trailing comma


# ---- the reference's own SAM files, round trip ------------------------------------------------------------------------------------------
def _int_tag(key, v):
    for ty, lo, hi in (("C", 0, 255), ("c", -128, 127), ("S", 0, 65535), ("s", -32768, 32767), ("I", 0, 2 ** 32 - 1), ("i", -2 ** 31, 2 ** 31 - 1)):
        if lo <= v <= hi:
            return bamgen.tag_num(key, ty, v)
    raise ValueError(v)


def sam_to_bam(sam_path, bam_path):
    """the SAM file as a BAM (bamgen); returns its record lines"""
    text, refs, recs, lines = "", [], [], []
    for line in open(sam_path).read().splitlines():
        if line.startswith("@"):
            text += line + "\n"
            if line.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in line.split("\t")[1:])
                refs.append((f["SN"], int(f["LN"])))
            continue
        lines.append(line)
        f = line.split("\t")
        ids = {n: k for k, (n, _) in enumerate(refs)}
        r = ids.get(f[2], -1)
        m = r if f[6] == "=" else ids.get(f[6], -1)
        tags = b""
        for t in f[11:]:
            key, ty, val = t.split(":", 2)
            tags += {"i": lambda: _int_tag(key, int(val)), "Z": lambda: bamgen.tag_z(key, val), "A": lambda: bamgen.tag_num(key, "A", val),
                     "f": lambda: bamgen.tag_num(key, "f", float(val))}[ty]()
        seq = "" if f[9] == "*" else f[9]
        qual = [0xFF] * len(seq) if f[10] == "*" else [ord(c) - 33 for c in f[10]]
        recs.append(bamgen.make_record(r, int(f[3]) - 1, "" if f[5] == "*" else f[5], seq, qual, name=f[0], mapq=int(f[4]), flag=int(f[1]), tags=tags,
                                       next_ref=m, next_pos=int(f[7]) - 1, tlen=int(f[8])))
    bamgen.write_bam(bam_path, refs, recs, text=text, write_index=False)
    return lines


@pytest.mark.parametrize("name", ["issue_356.sam", "ex1_header_500.sam"])
def test_reference_sam_round_trip(name, tmp_path):
    bam = str(tmp_path / "rt.bam")
    lines = sam_to_bam(os.path.join(GOLDEN, name), bam)
    got, st = view_sam(bam, tmp_path)
    want = "".join(l + "\n" for l in lines).encode()
    assert len(lines) > 10 and st["n_entries_out"] == len(lines)
    assert got == want, first_difference(got, want)


# ---- pieces ---------------------------------------------------------------------------------------------------------------------------
def test_pieces_do_not_change_a_byte(edges, tmp_path, monkeypatch, capfd):
    path, want = edges
    lines = want.split(b"\n")[:-1]
    longest = max(len(l) + 1 for l in lines)
    two = len(lines[0]) + len(lines[1]) + 2               # the first piece ends exactly on the end of the second line
    assert longest > 64 * 1000                             # one line is longer than the small budgets
    monkeypatch.setenv("SBX_TIMING", "1")
    for budget in ("1", "64", str(len(lines[0]) + 1), str(two), str(longest), "not a number", None):
        if budget is None:
            monkeypatch.delenv("SBX_SAM_PIECE_BYTES", raising=False)
        else:
            monkeypatch.setenv("SBX_SAM_PIECE_BYTES", budget)
        capfd.readouterr()
        got, _ = view_sam(path, tmp_path, tag="p")
        err = capfd.readouterr().err
        assert got == want, (budget, first_difference(got, want))
        line = [x for x in err.splitlines() if x.startswith("[sbx] output: text_bytes=")]
        assert len(line) == 1 and "text_bytes=%d " % len(want) in line[0], err[-500:]
        # the pieces are the greedy cut at line ends: as many lines as fit the budget, at least one
        cap = int(budget) if budget and budget.isdigit() else 64 << 20
        pieces, used = 1, 0
        for l in lines:
            if used and used + len(l) + 1 > cap:
                pieces, used = pieces + 1, 0
            used += len(l) + 1
        assert int(line[0].split("n_pieces=")[1].split()[0]) == pieces, budget
        assert pieces == {"1": len(lines), None: 1}.get(budget, pieces)
        view = [x for x in err.splitlines() if x.startswith("[sbx] view:")]
        assert len(view) == 1 and "sink=sam" in view[0] and "ms_gather=" in view[0] and "compressed_bytes=0 " in view[0]


# ---- batches, listed regions, the other parts of the selection ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ties(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("samties") / "ties.bam")
    info = bamgen.write_bam(path, TIE_REFS, _tie_records(n=1500, seed=31), text=UNSORTED, block_size=4000, write_index=False)
    return path, info


LISTED = ["c1:1-200", "c1:50-150", "c2", "c1:1-200", "*"]


def _keep_q30_not_dup(rec):
    bin_mq_nl, flag_nc = struct.unpack_from("<II", rec, 12)
    return ((bin_mq_nl >> 8) & 0xFF) >= 30 and not (flag_nc >> 16) & 0x400


def test_batches_and_overlapping_listed_regions(ties, tmp_path, monkeypatch):
    path, info = ties
    want, n = expected_text(path, regions=LISTED)
    one, st1 = view_sam(path, tmp_path, regions=LISTED)
    assert one == want, first_difference(one, want)
    assert st1["n_batches"] == 1 and st1["n_entries_out"] == n > st1["n_records_selected"]      # records are printed several times
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", str(info["stream_len"] // 5))
    monkeypatch.setenv("SBX_SAM_PIECE_BYTES", "5000")
    many, st = view_sam(path, tmp_path, tag="b", regions=LISTED)
    assert st["n_batches"] >= 3 and st["n_sort_passes"] >= 1
    assert many == want, first_difference(many, want)
    rev, _ = view_sam(path, tmp_path, tag="r", regions=LISTED[::-1])
    assert rev == expected_text(path, regions=LISTED[::-1])[0] and rev != want and sorted(rev.split(b"\n")) == sorted(want.split(b"\n"))


@pytest.mark.parametrize("kind", ["bed", "subsample", "num_filter", "filter"])
def test_the_other_parts_of_the_selection(ties, tmp_path, kind):
    path, _ = ties
    kw, sel = {}, {}
    if kind == "bed":
        lines = ["c1\t49\t150", "c2\t0\t20000", "chrNotThere\t0\t10"]
        bed = str(tmp_path / "s.bed")
        open(bed, "w").write("".join(l + "\n" for l in lines))
        kw, sel = dict(bed=bed), dict(bed_lines=lines)
    elif kind == "subsample":
        kw = sel = dict(subsample=0.25, seed=7)
    elif kind == "num_filter":
        kw = sel = dict(num_filter="/16")
    else:
        kw, sel = dict(filter="mapping_quality >= 30 and not duplicate"), dict(keep=_keep_q30_not_dup)
    want, n = expected_text(path, **sel)
    got, st = view_sam(path, tmp_path, **kw)
    assert 0 < n < st["n_records_in"] and st["n_entries_out"] == n
    assert got == want, first_difference(got, want)


# ---- -h ---------------------------------------------------------------------------------------------------------------------------------
def test_header(ties, tmp_path):
    import sambamba_amd
    path, _ = ties
    want, _ = expected_text(path, regions=["c2"])
    header = sambamba_amd.markdup_header_text(UNSORTED, "view -h it")
    assert "@PG\tID:sambamba\tCL:view -h it" in header
    got, _ = view_sam(path, tmp_path, regions=["c2"], with_header=True, command_line="view -h it")
    assert got == header.encode() + want                 # no blank line between them
    got, _ = view_sam(path, tmp_path, regions=["c2"], command_line="view -h it")
    assert got == want
    # an empty selection writes the header or nothing
    got, st = view_sam(path, tmp_path, filter="mapping_quality > 254", with_header=True, command_line="view -h it")
    assert got == header.encode() and st["n_entries_out"] == 0 and st["stream_bytes"] == 0
    got, _ = view_sam(path, tmp_path, filter="mapping_quality > 254")
    assert got == b""
    empty = str(tmp_path / "empty.bam")
    bamgen.write_bam(empty, TIE_REFS, [], text=UNSORTED, write_index=False)
    got, st = view_sam(empty, tmp_path, tag="e", with_header=True)
    assert got == sambamba_amd.markdup_header_text(UNSORTED, None).encode() and st["n_records_in"] == 0


# ---- malformed records ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(cases.malformed_records()))
def test_malformed_records_are_an_error_code(case, tmp_path):
    import sambamba_amd
    bad = cases.malformed_records()[case]
    # the bad record carries flag bit 0x200 so that --num-filter can leave it out
    bad = bad[:18] + struct.pack("<H", struct.unpack_from("<H", bad, 18)[0] | 0x200) + bad[20:]
    recs = [cases.good_record(k) for k in range(300)]
    recs.insert(170, bad)
    path = str(tmp_path / "bad.bam")
    bamgen.write_bam(path, cases.REFS, recs, text=cases.TEXT, write_index=False)
    out = str(tmp_path / "bad.sam")
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(path, out, format="sam")
    assert ei.value.code == -3 and "(1 records" in ei.value.msg and not os.path.exists(out)
    r = cli(["-o", out, path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"sbx-sam: malformed BAM record") and not os.path.exists(out)
    if case == "ref_id_is_n_ref":
        return              # (the read pass refuses this one for every sink, selected or not: tests/test_gpu_view.py)
    # not selected: no error, and the lines of the others
    got, st = view_sam(path, tmp_path, num_filter="/512")
    want = sam_ref.sam_text([r_ for r_ in recs if r_ is not bad], cases.REF_NAMES)
    assert st["n_entries_out"] == 300 and got == want


# ---- the command line ---------------------------------------------------------------------------------------------------------------------
def test_sbx_sam_command_line(ties, tmp_path):
    from sambamba_amd import view_cli_path
    from tests.test_gpu_sort import check_file
    path, _ = ties
    want, _ = expected_text(path, regions=["c2"])
    for args in ([path, "c2"], ["-f", "sam", path, "c2"], ["--format=sam", "-o", "-", path, "c2"]):
        r = cli(args)
        assert r.returncode == 0 and r.stdout == want, r.stderr[-500:]
    out = str(tmp_path / "o.sam")
    args = ["-h", "-o", out, path, "c2"]
    r = cli(args)
    import sambamba_amd
    assert r.returncode == 0 and r.stdout == b"", r.stderr[-500:]
    assert open(out, "rb").read() == sambamba_amd.markdup_header_text(UNSORTED, "view " + " ".join(args)).encode() + want
    # -f bam still works, -c too
    outb = str(tmp_path / "o.bam")
    args = ["-f", "bam", "-l", "1", "-o", outb, path, "c2"]
    r = cli(args)
    assert r.returncode == 0, r.stderr[-500:]
    stream = inflate(path)
    check_file(outb, ref.expected_stream(stream, "view " + " ".join(args), regions=[ref.parse_region("c2", ref.refs_of(stream))]))
    r = cli(["-c", path, "c2"])
    assert r.returncode == 0 and r.stdout == b"%d\n" % want.count(b"\n")
    # -l with SAM output is refused, the other formats are still refused by name
    r = cli(["-l", "3", "-o", out + "2", path])
    assert r.returncode == 1 and r.stdout == b"" and r.stderr.startswith(b"sbx-sam: -l") and not os.path.exists(out + "2")
    r = cli(["-f", "json", path])
    assert r.returncode == 1 and r.stderr == b"sbx-sam: output format json is not supported yet: use -f bam or -c\n"
    # the output must not be the input; a failure leaves no file
    r = cli(["-o", path, path])
    assert r.returncode == 1 and r.stderr.startswith(b"sbx-sam: the output would overwrite the input")
    r = cli(["-o", out + "3", path, "chrNotThere"])
    assert r.returncode == 1 and b"chrNotThere" in r.stderr and not os.path.exists(out + "3")
    # usage
    r = cli([])
    assert r.returncode == 0 and r.stdout == b"" and r.stderr.startswith(b"Usage: sbx-sam [options] <input.bam> [region1 [...]]\n")
    assert b"-f, --format=sam|bam" in r.stderr and b"(default: sam)" in r.stderr and b"print header before reads" in r.stderr
    # sbx-view is as it was: sam is refused by name
    for args in (["-f", "sam", path], [path]):
        r = cli(args, exe=view_cli_path())
        assert r.returncode == 1 and r.stdout == b"" and r.stderr == b"sbx-view: output format sam is not supported yet: use -f bam or -c\n"


# ---- the Python API -----------------------------------------------------------------------------------------------------------------------
def test_python_api(ties, tmp_path):
    import sambamba_amd
    path, _ = ties
    out = str(tmp_path / "api.sam")
    for kw in (dict(level=1), dict(index=True), dict(level=0, index=True)):
        with pytest.raises(ValueError):
            sambamba_amd.view(path, out, format="sam", **kw)
    with pytest.raises(ValueError):
        sambamba_amd.view(path, out, format="json")
    assert not os.path.exists(out)
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.view(path, path, format="sam")
    assert ei.value.code == -1
    # the default is still a BAM
    sambamba_amd.view(path, out, regions=["c2"])
    assert open(out, "rb").read(4) == b"\x1f\x8b\x08\x04"
    assert "sbx_view_sam" in sambamba_amd._lib.EXPORTS and os.path.exists(sambamba_amd.sam_cli_path())


# ---- the offsets of the lines (launch_group_offsets) at the edges of the workgroup of 256 ----
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_entry_counts_around_the_offset_group(n, tmp_path):
    pool = cases.edge_records() + cases.tag_records()
    recs = [pool[k % len(pool)] for k in range(n)]
    path = str(tmp_path / "n.bam")
    bamgen.write_bam(path, cases.REFS, recs, text=cases.TEXT, write_index=False)
    want, n_want = expected_text(path)
    got, st = view_sam(path, tmp_path)
    assert got == want, first_difference(got, want)
    assert n_want == st["n_entries_out"] == n and st["stream_bytes"] == len(want)
