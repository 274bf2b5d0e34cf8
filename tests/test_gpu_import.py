"""sbx_import_sam / sambamba_amd.import_sam / sbx-import on the device: SAM text parsed into BAM records by K15 (samparse.hip), against
the Python restatement of the grammar (tests/samin_ref.py) and through the project's own SAM writer and back."""
import os
import random
import subprocess

import pytest

from tests import bamgen
from tests import sam_cases
from tests import sam_ref
from tests import samin_cases as cases
from tests import samin_ref as ref
from tests.flagstat_ref import inflate
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

N_HEADER_LINES = cases.TEXT.count("\n")


def first_difference(got, want):
    k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    return "lengths %d / %d, first difference at byte %d: %r / %r" % (len(got), len(want), k, got[max(0, k - 40):k + 40], want[max(0, k - 40):k + 40])


def do_import(data, tmp_path, tag="i", **kw):
    """(path of the BAM, stats) of import_sam over these SAM bytes"""
    import sambamba_amd
    sam, bam = str(tmp_path / (tag + ".sam")), str(tmp_path / (tag + ".bam"))
    with open(sam, "wb") as f:
        f.write(data)
    return bam, sambamba_amd.import_sam(sam, bam, **kw)


def expected_stream(data, command_line=None):
    """the inflated BAM the restatement gives for these SAM bytes"""
    import sambamba_amd
    text, lines = ref.split_sam(data)
    refs = ref.header_references(text)
    names = [n for n, _ in refs]
    return ref.bam_stream(sambamba_amd.markdup_header_text(text, command_line), refs, [ref.record(l, names) for l in lines])


def refused(data, tmp_path, tag="bad"):
    """the SbxError of an import that must fail; no output file may be left"""
    import sambamba_amd
    with pytest.raises(sambamba_amd.SbxError) as ei:
        do_import(data, tmp_path, tag=tag)
    assert not os.path.exists(str(tmp_path / (tag + ".bam")))
    return ei.value


# ---- every field and every tag type at its edges ------------------------------------------------------------------------------------
def test_edge_lines(tmp_path):
    data = cases.sam_text(list(cases.good_lines().values()))
    bam, st = do_import(data, tmp_path)
    got, want = inflate(bam), expected_stream(data)
    assert got == want, first_difference(got, want)        # header text, reference list and every record
    assert st["n_records"] == st["n_lines"] == len(cases.good_lines()) and st["n_chunks"] == 1
    assert st["text_bytes"] == len(data) - len(cases.TEXT) and st["stream_bytes"] == len(want)


# ---- newlines on every lane, wave and workgroup boundary of K15a; one line longer than 250,000 bytes ------------------------------
def _line_of(length, k):
    """an unmapped line of exactly `length` bytes, its '\\n' included (length >= 22)"""
    extra = length - 22
    name = b"a"
    if extra < 250:
        return cases.line(name + b"n" * extra, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"*", b"*")
    if extra % 2 == 0 and k % 2 == 0:                      # SEQ and QUAL of n bases replace the two '*'
        n = (extra + 2) // 2
        return cases.line(name, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", bytes(b"ACGTN"[j % 5] for j in range(n)), bytes(33 + j % 94 for j in range(n)))
    return cases.line(name, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"*", b"*", [b"XZ:Z:" + b"z" * (extra - 6)])


@pytest.fixture(scope="module")
def boundary_lines():
    lengths = list(range(22, 701))
    order = (lengths * 5)[:3000]
    random.Random(20241018).shuffle(order)
    lines = [_line_of(n, k) for k, n in enumerate(order)]
    assert all(len(l) + 1 == n for l, n in zip(lines, order))
    n_long = 130000
    long_line = cases.line(b"long", cigar=b"%dM" % n_long, seq=b"ACGT" * (n_long // 4), qual=b"5" * n_long, tags=[b"NM:i:0"])
    assert len(long_line) > 250000
    lines.insert(1500, long_line)
    return lines


@pytest.fixture(scope="module")
def boundary_default(boundary_lines, tmp_path_factory):
    """the file with a final newline, imported with the default chunk size: (SAM bytes, BAM file bytes)"""
    data = cases.sam_text(boundary_lines)
    bam, st = do_import(data, tmp_path_factory.mktemp("importb"), tag="default")
    assert st["n_chunks"] == 1
    return data, open(bam, "rb").read()


@pytest.mark.parametrize("final_newline", [False, True])
def test_line_index_boundaries(boundary_lines, final_newline, tmp_path):
    data = cases.sam_text(boundary_lines, final_newline=final_newline)
    bam, st = do_import(data, tmp_path)
    got, want = inflate(bam), expected_stream(data)
    assert st["n_records"] == st["n_lines"] == len(boundary_lines)
    assert got == want, first_difference(got, want)


# ---- the chunk size does not change a byte ------------------------------------------------------------------------------------------
def _greedy_chunks(lines, budget):
    n, used = 0, 0
    for l in lines:
        if used and used + len(l) + 1 > budget:
            n, used = n + 1, 0
        used += len(l) + 1
    return n + (1 if used else 0)


def test_chunks_do_not_change_a_byte(boundary_lines, boundary_default, tmp_path, monkeypatch):
    data, want_file = boundary_default
    longest = max(len(l) + 1 for l in boundary_lines)
    for budget in (1, 4096, longest - 1, longest + 1):
        monkeypatch.setenv("SBX_IMPORT_CHUNK_BYTES", str(budget))
        bam, st = do_import(data, tmp_path, tag="c%d" % budget)
        got_file = open(bam, "rb").read()
        assert got_file == want_file, (budget, first_difference(got_file, want_file))
        assert st["n_chunks"] == _greedy_chunks(boundary_lines, budget), budget
    assert _greedy_chunks(boundary_lines, 1) == len(boundary_lines) and _greedy_chunks(boundary_lines, longest + 1) > 2


# ---- through the project's own tools ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["issue_356.sam", "ex1_header_500.sam"])
def test_golden_sam_round_trip(name, tmp_path):
    import sambamba_amd
    data = open(os.path.join(GOLDEN, name), "rb").read()
    _, lines = ref.split_sam(data)
    bam, out = str(tmp_path / "g.bam"), str(tmp_path / "g.sam")
    st = sambamba_amd.import_sam(os.path.join(GOLDEN, name), bam)
    sambamba_amd.view(bam, out, format="sam", with_header=False)
    got, want = open(out, "rb").read(), b"".join(l + b"\n" for l in lines)
    assert st["n_records"] == len(lines) > 10
    assert got == want, first_difference(got, want)


def test_text_fixed_point(tmp_path):
    """records -> text -> records -> text: the two texts are equal.  The record BYTES may differ -- an integer tag comes back in the
    smallest type, the bin is recomputed -- which is why the texts are compared."""
    import sambamba_amd
    recs = sam_cases.edge_records() + sam_cases.tag_records()
    # records whose own SAM text lies outside the grammar cannot come back: an empty QNAME (l_read_name 0 and 1), CIGAR operation
    # codes above 8 ('?'), a POS that wraps to a negative number, a quality that prints as a space, a Z and an H tag with no byte
    # of value (the grammar's Z and H are one byte or more)
    outside = {}
    for r in recs:
        text = sam_ref.sam_line(r, sam_cases.REF_NAMES).rstrip(b"\n")
        try:
            ref.record(text, sam_cases.REF_NAMES)
        except ref.Malformed:
            outside[text.split(b"\t")[0]] = outside.get(text.split(b"\t")[0], 0) + 1
    assert outside == {b"": 2, b"cigops": 1, b"pos2": 1, b"qlate": 1, b"scalars": 1}
    keep = [r for r in recs if sam_ref.sam_line(r, sam_cases.REF_NAMES).split(b"\t")[0] not in outside]
    first_bam, first, second_bam, second = (str(tmp_path / n) for n in ("a.bam", "a.sam", "b.bam", "b.sam"))
    bamgen.write_bam(first_bam, sam_cases.REFS, keep, text=sam_cases.TEXT, write_index=False)
    sambamba_amd.view(first_bam, first, format="sam", with_header=True)
    st = sambamba_amd.import_sam(first, second_bam)
    sambamba_amd.view(second_bam, second, format="sam", with_header=True)
    a, b = open(first, "rb").read(), open(second, "rb").read()
    assert st["n_records"] == len(keep) > 25
    assert a == b, first_difference(b, a)


# ---- malformed input ----------------------------------------------------------------------------------------------------------------
def test_every_malformed_line_is_refused(tmp_path):
    good = [cases.line(b"g%d" % k) for k in range(6)]
    for j, (name, bad) in enumerate(cases.malformed_lines().items()):
        at = j % 5 + 1                                       # good lines in front of the bad one
        e = refused(cases.sam_text(good[:at] + [bad] + good[at:]), tmp_path, tag="m%d" % j)
        k = N_HEADER_LINES + at + 1
        assert e.code == -3, name
        assert ": 1 line is outside the grammar" in str(e) and str(e).endswith("the first is line %d" % k), (name, str(e))


def test_two_malformed_lines(tmp_path):
    good = [cases.line(b"g%d" % k) for k in range(600)]
    bad = cases.malformed_lines()
    lines = good[:300] + [bad["qual_short"]] + good[300:] + [bad["tag_i_2_32"]]
    e = refused(cases.sam_text(lines, final_newline=False), tmp_path)
    assert e.code == -3 and ": 2 lines are outside the grammar" in str(e) and str(e).endswith("the first is line %d" % (N_HEADER_LINES + 301))


# ---- small inputs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", [b"", cases.TEXT.encode(), cases.TEXT.encode().rstrip(b"\n")], ids=["zero_bytes", "header_only", "header_without_newline"])
def test_no_records(data, tmp_path):
    import sambamba_amd
    bam, st = do_import(data, tmp_path)
    assert st["n_records"] == st["n_lines"] == 0
    got, want = inflate(bam), expected_stream(data)
    assert got == want, first_difference(got, want)
    assert open(bam, "rb").read().endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))      # the EOF block
    assert sambamba_amd.flagstat(bam)["reads"] == (0, 0)


def test_no_reference_table(tmp_path):
    unmapped = [cases.line(b"u%d" % k, b"4", b"*", b"0", b"0", b"*", b"*", b"0", b"0", b"ACGT", b"IIII") for k in range(3)]
    data = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join(l + b"\n" for l in unmapped)
    bam, st = do_import(data, tmp_path)
    assert st["n_records"] == 3 and inflate(bam) == expected_stream(data)
    e = refused(data + cases.line(b"m") + b"\n", tmp_path)
    assert e.code == -3 and str(e).endswith("the first is line 5")
    # no header at all
    bam, st = do_import(b"".join(l + b"\n" for l in unmapped), tmp_path, tag="nohdr")
    assert st["n_records"] == 3


# ---- the command line and the options -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sorted_sam(tmp_path_factory):
    """a coordinate-sorted SAM file: path, bytes"""
    rng = random.Random(7)
    lines = []
    for r, (name, length) in enumerate(cases.REFS):
        for p in sorted(rng.randrange(1, length - 200) for _ in range(400)):
            lines.append(cases.line(b"s%d_%d" % (r, p), b"0", name.encode(), b"%d" % p, b"40", b"50M", b"*", b"0", b"0", b"ACGTA" * 10, b"F" * 50, [b"NM:i:%d" % (p % 7)]))
    data = cases.TEXT.replace("SO:unsorted", "SO:coordinate").encode() + b"".join(l + b"\n" for l in lines)
    path = str(tmp_path_factory.mktemp("importsorted") / "sorted.sam")
    with open(path, "wb") as f:
        f.write(data)
    return path, data


def test_levels_and_index(sorted_sam, tmp_path):
    import sambamba_amd
    path, data = sorted_sam
    streams = []
    for level in (0, 1, 9):
        out = str(tmp_path / ("l%d.bam" % level))
        sambamba_amd.import_sam(path, out, level=level)
        streams.append(inflate(out))
    assert streams[0] == streams[1] == streams[2] == expected_stream(data)
    out = str(tmp_path / "ix.bam")
    sambamba_amd.import_sam(path, out, index=True, command_line="view -S x")
    assert inflate(out) == expected_stream(data, "view -S x")
    sambamba_amd.build_index(out, str(tmp_path / "own.bai"))
    assert open(out + ".bai", "rb").read() == open(str(tmp_path / "own.bai"), "rb").read()
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.import_sam(path, path)
    assert ei.value.code == -1 and open(path, "rb").read() == data


def test_command_line(sorted_sam, tmp_path):
    import sambamba_amd
    path, data = sorted_sam
    imp = sambamba_amd.import_cli_path()
    # -o - and no -o: the BAM on stdout
    r = subprocess.run([imp, "-S", "-f", "bam", "-o", "-", path], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()
    via_stdout = str(tmp_path / "stdout.bam")
    open(via_stdout, "wb").write(r.stdout)
    assert inflate(via_stdout) == expected_stream(data, "view -S -f bam -o - " + path)
    # sbx-sam in.bam | sbx-import -o out.bam -
    bam, out = str(tmp_path / "in.bam"), str(tmp_path / "piped.bam")
    sambamba_amd.import_sam(path, bam)
    p1 = subprocess.Popen([sambamba_amd.sam_cli_path(), "-h", bam], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p2 = subprocess.run([imp, "-l", "1", "-o", out, "-"], stdin=p1.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p1.stdout.close()
    assert p1.wait() == 0 and p2.returncode == 0, (p1.stderr.read().decode(), p2.stderr.decode())
    text = subprocess.run([sambamba_amd.sam_cli_path(), "-h", bam], stdout=subprocess.PIPE).stdout
    assert inflate(out) == expected_stream(text, "view -l 1 -o %s -" % out)
    # a malformed line: status 1, the message, no file
    bad = str(tmp_path / "bad.sam")
    open(bad, "wb").write(data + b"not a line\n")
    r = subprocess.run([imp, "-o", str(tmp_path / "bad.bam"), bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and r.stderr.decode().startswith("sbx-import: malformed SAM text") and not os.path.exists(str(tmp_path / "bad.bam"))


# ---- the scans behind K15a and K15b (launch_scan64, launch_group_offsets) at the edges of the workgroup of 256 lines ----
@pytest.mark.parametrize("final_newline", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_line_counts_around_the_offset_group(n, final_newline, tmp_path):
    lines = [_line_of(22 + (37 * k) % 300, k) for k in range(n)]
    data = cases.sam_text(lines, final_newline=final_newline)
    bam, st = do_import(data, tmp_path)
    got, want = inflate(bam), expected_stream(data)
    assert st["n_records"] == st["n_lines"] == n and st["n_chunks"] == 1
    assert got == want, first_difference(got, want)


def test_input_that_ends_at_a_chunk_end(tmp_path, monkeypatch):
    """every chunk is filled to its last byte, so the reader meets the end of the input with an empty slot in its hands"""
    lines = [_line_of(100, k) for k in range(6)]
    data = cases.sam_text(lines)
    monkeypatch.delenv("SBX_IMPORT_CHUNK_BYTES", raising=False)
    want = inflate(do_import(data, tmp_path, tag="default")[0])
    assert want == expected_stream(data)
    for per_chunk in (6, 2, 1):
        monkeypatch.setenv("SBX_IMPORT_CHUNK_BYTES", str(100 * per_chunk))
        bam, st = do_import(data, tmp_path, tag="c%d" % per_chunk)
        assert st["n_chunks"] == 6 // per_chunk and st["n_records"] == 6 and st["text_bytes"] == 600
        assert inflate(bam) == want
