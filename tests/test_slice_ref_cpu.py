"""tests/slice_ref.py -- the Python restatement of what `sbx-slice` writes -- on hand-made files with known answers, among them the two
places where the reference's code departs from its own header comment and this project follows the comment.  No GPU needed."""
from tests import bamgen
from tests.slice_ref import Bam, slice_ref

REFS = [("chr1", 100000), ("chr2", 50000), ("chr3", 50000)]


def rec(ref, pos, cigar, name, flag=0):
    n = sum(k for op, k in bamgen.parse_cigar(cigar) if op in "MIS=X")
    return bamgen.make_record(ref, pos, cigar, "A" * n, 30, name=name, flag=flag)


def names(records):
    return [r[36:36 + r[12] - 1].decode() for r in records]


def make(tmp_path, recs, **kw):
    path = str(tmp_path / "in.bam")
    bamgen.write_bam(path, REFS, recs, write_index=False, **kw)
    return path


def test_r1_then_the_stretch_between_the_two_first_ge(tmp_path):
    recs = [rec(0, 100, "50M", "before"), rec(0, 180, "50M", "reaches"), rec(0, 200, "50M", "at_beg"), rec(0, 250, "10M", "inside"),
            rec(0, 299, "50M", "last_inside"), rec(0, 300, "50M", "at_end"), rec(1, 10, "50M", "next_contig"), rec(-1, -1, "", "unplaced", flag=4)]
    path = make(tmp_path, recs, block_size=150)
    stream, verbatim, per = slice_ref(path, ["chr1:201-300"])
    assert names(per[0]) == ["reaches", "at_beg", "inside", "last_inside"]
    bam = Bam(path)
    assert stream == bam.stream[:bam.header_len] + recs[1] + recs[2] + recs[3] + recs[4]
    # the whole blocks between the start of at_beg and the start of at_end, and only those
    a, b = bam.u[2], bam.u[5]
    assert verbatim[0] and len(b"".join(verbatim[0])) > 0
    assert len(verbatim[0]) == sum(1 for k in range(len(bam.blocks)) if a <= bam.block_start[k] and bam.block_start[k + 1] <= b)
    # regions in the order given, common records twice; a contig without reads; a contig followed by reads without reference; "*"
    _, _, per = slice_ref(path, ["chr1:251-400", "chr1:201-300", "chr3", "chr2"])
    assert [names(p) for p in per] == [["inside", "last_inside", "at_end"], ["reaches", "at_beg", "inside", "last_inside"], [], ["next_contig"]]
    stream, _, per = slice_ref(path, ["*"])
    assert names(per[0]) == ["unplaced"] and stream == bam.stream[:bam.header_len] + recs[7]


def test_a_record_without_cigar_at_beg_is_in_the_stretch_and_not_in_r1(tmp_path):
    recs = [rec(0, 150, "40M", "short"), rec(0, 199, "", "no_cigar_before"), rec(0, 200, "", "no_cigar_at_beg"), rec(0, 200, "5M", "mapped_at_beg")]
    _, _, per = slice_ref(make(tmp_path, recs), ["chr1:201-300"])
    assert names(per[0]) == ["no_cigar_at_beg", "mapped_at_beg"]


def test_divergence_1_records_behind_the_last_r1_record_that_do_not_reach_beg(tmp_path):
    """slice.d's loop starts the copy at the end of the last R1 record, so `short_behind` -- it starts in front of beg, behind the R1
    record `long`, and ends in front of beg -- would be copied by the reference's code.  The header comment defines s2_start_offset as
    the first read with position >= beg: it is not part of the slice."""
    recs = [rec(0, 100, "200M", "long"), rec(0, 150, "10M", "short_behind"), rec(0, 200, "50M", "first_in_region"), rec(0, 400, "10M", "behind")]
    _, _, per = slice_ref(make(tmp_path, recs), ["chr1:201-300"])
    assert names(per[0]) == ["long", "first_in_region"]
    assert "short_behind" not in names(per[0])


def test_divergence_2_reads_reach_end_and_none_of_the_contig_starts_behind_it(tmp_path):
    """reads2 = reference[end .. max] holds `reaches_end` only (it overlaps end and starts in front of it); slice.d's loop leaves
    s2_end_offset at the start of that read and loses it.  The comment's case 3 ends the stretch behind the last read of the contig."""
    recs = [rec(0, 210, "10M", "inside"), rec(0, 280, "50M", "reaches_end"), rec(1, 5, "10M", "next_contig")]
    _, _, per = slice_ref(make(tmp_path, recs), ["chr1:201-300"])
    assert names(per[0]) == ["inside", "reaches_end"]


def test_a_read_far_in_front_of_beg_is_in_r1(tmp_path):
    recs = [rec(0, 1000, "100M30000N100M", "spliced"), rec(0, 1200, "50M", "near"), rec(0, 31050, "50M", "in_region")]
    _, _, per = slice_ref(make(tmp_path, recs), ["chr1:31051-31100"])
    assert names(per[0]) == ["spliced", "in_region"]
