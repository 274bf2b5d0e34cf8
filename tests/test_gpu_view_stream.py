"""The streamed sinks of `view` (sbx_view_run_streamed).  BAM: K21 of stream.hip and the StreamedOutput of engine_streamout.hpp -- no
record store; every batch of the read pass is packed, while it is on the device, into one staging window that goes to the BGZF
encoder.  SAM: no store either; K12b, K13a and K13b run per batch over the records where K1 left them.

Every case writes the output once on the resident path (SBX_STREAM_WINDOW_BYTES unset) and once streamed with a window of one
65280-byte piece, and asserts that the two FILES are identical, that the streamed stats report the expected number of windows, and
that the resident output is what tests/view_ref.py expects.  On a library without the feature the hook is ignored and no stream
stats exist: the n_windows assertions fail."""
import filecmp
import os
import random
import struct

import pytest

from tests import bamgen
from tests import sam_cases
from tests import sam_ref
from tests import view_ref as ref
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream
from tests.test_gpu_sort import REFS, UNSORTED, _tie_records, check_file

pytestmark = pytest.mark.gpu

PIECE = 0xFF00
BLOCK = 700            # payload bytes per BGZF block of the generated inputs: records straddle the blocks
BATCH = "20000"        # SBX_INDEX_BATCH_BYTES: the generated inputs come in five or more batches


def windows_of(n_bytes):
    return max(1, -(-n_bytes // PIECE))


def both(monkeypatch, path, tmp_path, tag="o", want=None, batch=BATCH, streamed_windows=True, **kw):
    """view(path, ...) resident, then streamed; the files compared; returns (resident stats, streamed stats, the file's bytes)"""
    import sambamba_amd
    monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES", raising=False)
    a, b = str(tmp_path / (tag + ".resident.bam")), str(tmp_path / (tag + ".streamed.bam"))
    st_r = sambamba_amd.view(path, a, **kw)
    monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", "1")
    st_s = sambamba_amd.view(path, b, **kw)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES")
    print("%s: stream_bytes %d n_batches %d n_windows %d n_pack_launches %d ms_pack %.3f" % (
        tag, st_s["stream_bytes"], st_s["n_batches"], st_s["n_windows"], st_s["n_pack_launches"], st_s["ms_pack"]))
    assert filecmp.cmp(a, b, shallow=False)
    assert (st_r["n_windows"], st_r["window_bytes"], st_r["n_pack_launches"], st_r["ms_pack"]) == (0, 0, 0, 0.0)
    if streamed_windows:
        assert st_s["n_windows"] == windows_of(st_s["stream_bytes"]) and st_s["window_bytes"] == PIECE
    for k in ("n_records_in", "n_records_selected", "n_entries_out", "stream_bytes", "compressed_bytes", "n_regions", "n_batches"):
        assert st_r[k] == st_s[k], k
    assert st_s["compressed_bytes"] == os.path.getsize(b)
    if want is not None:
        check_file(a, want)
    return st_r, st_s, open(b, "rb").read()


def expected(path, command_line=None, **sel):
    return ref.expected_stream(inflate(path), command_line, **sel)


@pytest.fixture(scope="module")
def ties(tmp_path_factory):
    """3000 short records in no order, blocks of 700 bytes"""
    path = str(tmp_path_factory.mktemp("viewstream") / "ties.bam")
    bamgen.write_bam(path, REFS, _tie_records(n=3000, seed=31), text=UNSORTED, block_size=BLOCK, write_index=False)
    return path


@pytest.fixture(scope="module")
def ordered(tmp_path_factory):
    """3000 records of c1 and c2 in coordinate order with a .bai, and 40 without a reference behind them"""
    path = str(tmp_path_factory.mktemp("viewstream") / "ordered.bam")
    rng = random.Random(5)
    recs = []
    for r, n in ((0, 2000), (1, 1000)):
        pos = 0
        for i in range(n):
            pos += rng.randrange(0, 40)
            recs.append(bamgen.make_record(r, pos, "10M", "ACGTACGTAC", 30, name="o%d_%05d" % (r, i), flag=0x10 if i % 3 == 0 else 0))
    recs += [bamgen.make_record(-1, -1, "", "ACGT", 30, name="u%03d" % i, flag=0x4, mapq=0) for i in range(40)]
    bamgen.write_bam(path, REFS, recs, block_size=BLOCK)
    return path


def _unmapped(rec):
    return bool(struct.unpack_from("<I", rec, 16)[0] >> 16 & 0x4)


def _mapq30(rec):
    return rec[13] >= 30


def test_small_windows_several_batches(ties, tmp_path, monkeypatch):
    """records cut by window ends, several windows inside one batch (a batch of 65 kB and more), several batches inside one window"""
    st_r, st_s, _ = both(monkeypatch, ties, tmp_path, want=expected(ties, "view all"), command_line="view all")
    assert st_s["n_windows"] >= 3 and st_s["n_batches"] >= 5
    assert st_s["n_pack_launches"] >= st_s["n_batches"]
    # a batch of several windows
    _, st_big, _ = both(monkeypatch, ties, tmp_path, tag="big", batch="150000", want=expected(ties))
    assert st_big["n_batches"] <= 2 and st_big["n_windows"] >= 3 and st_big["n_pack_launches"] >= st_big["n_windows"]
    # a selective -F: many batches go into one window
    _, st_f, _ = both(monkeypatch, ties, tmp_path, tag="sel", filter="unmapped", want=expected(ties, keep=_unmapped))
    assert st_f["n_batches"] >= 5 and st_f["n_windows"] == 1 and 0 < st_f["n_records_selected"] < st_f["n_records_in"] // 3
    _, st_q, _ = both(monkeypatch, ties, tmp_path, tag="q30", filter="mapping_quality >= 30", want=expected(ties, keep=_mapq30))
    assert st_q["n_windows"] >= 2


def test_window_size_does_not_change_the_file(ties, tmp_path, monkeypatch):
    import sambamba_amd
    _, _, raw = both(monkeypatch, ties, tmp_path)
    monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", BATCH)
    for hook, span in (("65281", 2 * PIECE), ("1000000", 16 * PIECE)):
        monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", hook)
        out = str(tmp_path / ("w%s.bam" % hook))
        st = sambamba_amd.view(ties, out)
        assert open(out, "rb").read() == raw
        # (a window is never larger than the stream in whole pieces)
        assert st["window_bytes"] == min(span, windows_of(st["stream_bytes"]) * PIECE)
        assert st["n_windows"] == -(-st["stream_bytes"] // st["window_bytes"])
    # anything that is not a positive decimal counts as unset
    for hook in ("0", "-1", "12k", ""):
        monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", hook)
        out = str(tmp_path / "unset.bam")
        st = sambamba_amd.view(ties, out)
        assert st["n_windows"] == 0 and open(out, "rb").read() == raw


def test_record_longer_than_a_window(tmp_path, monkeypatch):
    """one record with 150 k bases: about 225 kB, four windows and more, clipped at both ends in the middle ones"""
    rng = random.Random(2)
    long_seq = "".join(rng.choice("ACGT") for _ in range(150000))
    recs = [bamgen.make_record(0, 10 * i, "8M", "ACGTACGT", 30, name="s%03d" % i) for i in range(200)]
    recs.insert(100, bamgen.make_record(0, 1000, "150000M", long_seq, [rng.randrange(0, 60) for _ in range(150000)], name="long"))
    path = str(tmp_path / "long.bam")
    bamgen.write_bam(path, [("c1", 1000000), ("c2", 50000)], recs, write_index=False)
    want = expected(path)
    _, st, _ = both(monkeypatch, path, tmp_path, want=want)
    first = want.index(recs[100])
    assert (first + len(recs[100])) // PIECE - first // PIECE >= 3 and st["n_windows"] == windows_of(len(want)) >= 4


def test_long_header(tmp_path, monkeypatch):
    """a header longer than the first window: the first record starts in window 3"""
    refs = [("contig_number_%05d" % k, 1000 + k) for k in range(3000)]
    recs = [bamgen.make_record(i % 3000, 10, "8M", "ACGTACGT", 30, name="h%04d" % i) for i in range(1500)]
    path = str(tmp_path / "header.bam")
    info = bamgen.write_bam(path, refs, recs, block_size=BLOCK, write_index=False)
    want = expected(path, "view hdr")
    assert len(want) - sum(len(r) for r in recs) > 2 * PIECE and info["header_len"] > 2 * PIECE
    _, st, _ = both(monkeypatch, path, tmp_path, want=want, command_line="view hdr")
    assert st["n_windows"] >= 4
    # ... and nothing behind it
    _, st, _ = both(monkeypatch, path, tmp_path, tag="none", num_filter="2048", want=expected(path, bits=(2048, 0)))
    assert st["n_records_selected"] == 0 and st["n_windows"] >= 3 and st["n_pack_launches"] == 0


def test_nothing_selected(ties, tmp_path, monkeypatch):
    """header + EOF: one window, and no empty BGZF block in front of the EOF block (check_file)"""
    want = expected(ties, bits=(2048, 0))
    assert split_stream(want)[3] == []
    _, st, raw = both(monkeypatch, ties, tmp_path, num_filter="2048", want=want)
    assert st["n_windows"] == 1 and st["n_records_selected"] == 0 and st["n_pack_launches"] == 0
    assert raw.endswith(bamgen.EOF_BLOCK) and raw.count(bamgen.EOF_BLOCK[:16]) == 2


@pytest.mark.parametrize("extra", [0, 1])
def test_whole_windows(tmp_path, monkeypatch, extra):
    """header + records = 3 * 65280 exactly: three windows and nothing flushed short; one byte more: a fourth window of one byte"""
    recs = _tie_records(n=3200, seed=9)
    text = UNSORTED
    head = len(ref.expected_stream(bamgen.bam_header(text, REFS), None))
    size = head + sum(len(r) for r in recs)
    assert 2 * PIECE + 200 < size < 3 * PIECE - 200
    pad = 3 * PIECE + extra - size
    fill = bamgen.make_record(-1, -1, "", "ACGT", 30, name="fill", flag=0x4, tags=bamgen.tag_bytes("XB", bytes(pad)))
    fill = bamgen.make_record(-1, -1, "", "ACGT", 30, name="fill", flag=0x4, tags=bamgen.tag_bytes("XB", bytes(pad - (len(fill) - pad))))
    path = str(tmp_path / "whole.bam")
    bamgen.write_bam(path, REFS, recs + [fill], text=text, block_size=BLOCK, write_index=False)
    want = expected(path)
    assert len(want) == 3 * PIECE + extra                       # (checked on the CPU)
    _, st, _ = both(monkeypatch, path, tmp_path, want=want)
    assert st["stream_bytes"] == 3 * PIECE + extra and st["n_windows"] == 3 + extra


def test_a_batch_that_selects_nothing_and_an_empty_block(tmp_path, monkeypatch):
    """the records of the middle of the file are duplicates and --num-filter drops them: batches that select nothing lie between
    batches that do.  The last batch holds two BGZF blocks without payload: one more in front of the EOF block (the readers of
    this project, like tests.flagstat_ref.inflate, end the stream at the first block without payload, so such a block cannot lie
    in the middle of the records: the read pass refuses that file on the resident path too, "BAM record chain is broken")"""
    recs = []
    for i in range(3000):
        dup = 1000 <= i < 2000
        recs.append(bamgen.make_record(0, 10 + i, "8M", "ACGTACGT", 30, name="e%04d" % i, flag=0x400 if dup else 0))
    stream = bamgen.bam_header(UNSORTED, REFS) + b"".join(recs)
    blocks = [bamgen.bgzf_block(stream[o:o + BLOCK]) for o in range(0, len(stream), BLOCK)]
    blocks.append(bamgen.bgzf_block(b""))
    path = str(tmp_path / "gap.bam")
    with open(path, "wb") as fh:
        fh.write(b"".join(blocks) + bamgen.EOF_BLOCK)
    assert inflate(path) == stream
    want = ref.expected_stream(stream, None, bits=(0, 1024))
    _, st, _ = both(monkeypatch, path, tmp_path, num_filter="/1024", want=want)
    assert st["n_records_selected"] == 2000 and st["n_batches"] >= 6 and st["n_windows"] >= 2
    # (every batch that selects something is launched at least once; those of the middle are not)
    assert st["n_pack_launches"] <= (st["n_batches"] - 1) + (st["n_windows"] - 1)


def test_selections(ties, ordered, tmp_path, monkeypatch):
    refs = ref.refs_of(inflate(ties))
    both(monkeypatch, ties, tmp_path, tag="s", subsample=0.5, seed=77, want=expected(ties, subsample=(0.5, 77)))
    both(monkeypatch, ties, tmp_path, tag="nf", num_filter="/16", want=expected(ties, bits=(0, 16)))
    both(monkeypatch, ties, tmp_path, tag="one", regions=["c1:1-200"], want=expected(ties, regions=[ref.parse_region("c1:1-200", refs)]))
    _, st, _ = both(monkeypatch, ties, tmp_path, tag="c1", regions=["c1"], want=expected(ties, regions=[ref.parse_region("c1", refs)]))
    assert st["n_regions"] == 1 and st["n_windows"] >= 2
    _, st, _ = both(monkeypatch, ties, tmp_path, tag="star", regions=["*"], want=expected(ties, regions=["*"]))
    assert st["n_windows"] == 1 and st["n_records_selected"] > 0
    lines = ["c1\t49\t150", "c2\t0\t50000", "c1\t0\t200\tname", "chrNotThere\t0\t10"]
    bed = str(tmp_path / "sel.bed")
    open(bed, "w").write("".join(l + "\n" for l in lines))
    _, st, _ = both(monkeypatch, ties, tmp_path, tag="bed", bed=bed, filter="mapping_quality >= 30",
                    want=expected(ties, keep=_mapq30, bed=ref.merged_bed(lines, refs)))
    assert st["n_windows"] >= 2


def test_valid_only_leaves_the_invalid_record_out(tmp_path, monkeypatch):
    recs = _tie_records(n=2500, seed=3)
    bad = bamgen.make_record(0, 100, "4M", "ACGT", 30, name="not@valid")
    recs.insert(1700, bad)
    path = str(tmp_path / "v.bam")
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, block_size=BLOCK, write_index=False)
    want = expected(path, keep=lambda r: r != bad)
    st_r, st, _ = both(monkeypatch, path, tmp_path, valid=True, want=want)
    assert st["n_records_selected"] == len(recs) - 1 and st["n_windows"] >= 2


def test_indexed_pass(ordered, tmp_path, monkeypatch):
    """sbx-iview's pass: only the blocks the .bai names are read, on both paths"""
    refs = ref.refs_of(inflate(ordered))
    region = "c1:10000-30000"
    want = expected(ordered, regions=[ref.parse_region(region, refs)])
    st_r, st_s, _ = both(monkeypatch, ordered, tmp_path, regions=[region], use_index=True, want=want, batch="9000")
    assert st_s["blocks_read"] == st_r["blocks_read"] < st_r["blocks_in_file"] and st_s["runs"] == st_r["runs"]
    assert st_s["n_batches"] >= 3 and st_s["n_records_in"] < 3040


def test_two_listed_regions_keep_the_store(ties, tmp_path, monkeypatch):
    """the output is ordered by region: the resident path, whatever the hook says"""
    refs = ref.refs_of(inflate(ties))
    regions = ["c2", "c1:1-200"]
    want = expected(ties, regions=[ref.parse_region(r, refs) for r in regions])
    st_r, st_s, _ = both(monkeypatch, ties, tmp_path, regions=regions, want=want, streamed_windows=False)
    assert st_s["n_windows"] == 0 and st_s["n_pack_launches"] == 0 and st_s["n_sort_passes"] == st_r["n_sort_passes"] >= 1


def test_malformed_record_in_a_later_batch(tmp_path, monkeypatch):
    """a record whose reference id is out of range, far behind the first windows: the same code and message as on the resident
    path, and no output file although windows were written before it was met"""
    import sambamba_amd
    recs = _tie_records(n=3000, seed=13)
    recs[2800] = bamgen.make_record(7, 10, "4M", "ACGT", 30, name="badref")
    path = str(tmp_path / "bad.bam")
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, block_size=BLOCK, write_index=False)
    monkeypatch.setenv("SBX_BGZF_PIECE_BLOCKS", "1")
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", BATCH)
    seen = []
    for hook in (None, "1"):
        if hook:
            monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", hook)
        out = str(tmp_path / "bad.out.bam")
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.view(path, out)
        seen.append((ei.value.code, ei.value.msg))
        assert not os.path.exists(out)
    assert seen[0] == seen[1] and seen[0][0] == -3


def test_timing_line_and_entry_points(ties, tmp_path):
    import subprocess
    from sambamba_amd import view_cli_path
    out = str(tmp_path / "cli.bam")
    env = dict(os.environ, SBX_TIMING="1", SBX_BGZF_PIECE_BLOCKS="1", SBX_STREAM_WINDOW_BYTES="1", SBX_INDEX_BATCH_BYTES=BATCH)
    r = subprocess.run([view_cli_path(), "-f", "bam", "-o", out, ties], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0, r.stderr
    lines = [l for l in r.stderr.decode().splitlines() if l.startswith("[sbx] stream:")]
    assert len(lines) == 1
    fields = dict(f.split("=") for f in lines[0].split()[2:])
    assert set(fields) == {"n_windows", "window_bytes", "n_pack_launches", "ms_pack"}
    assert int(fields["n_windows"]) >= 3 and int(fields["window_bytes"]) == PIECE
    env.pop("SBX_STREAM_WINDOW_BYTES")
    r = subprocess.run([view_cli_path(), "-f", "bam", "-o", out + ".r", ties], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    assert r.returncode == 0 and b"[sbx] stream:" not in r.stderr


# ---- the SAM sink ----------------------------------------------------------------------------------------------------------------------
def both_sam(monkeypatch, path, tmp_path, tag="o", want=None, batch=BATCH, piece=None, streamed=True, **kw):
    """view(path, format="sam", ...) resident, then streamed; the texts compared; returns (resident stats, streamed stats, the text)"""
    import sambamba_amd
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", batch)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES", raising=False)
    if piece is None:
        monkeypatch.delenv("SBX_SAM_PIECE_BYTES", raising=False)
    else:
        monkeypatch.setenv("SBX_SAM_PIECE_BYTES", piece)
    a, b = str(tmp_path / (tag + ".resident.sam")), str(tmp_path / (tag + ".streamed.sam"))
    st_r = sambamba_amd.view(path, a, format="sam", **kw)
    monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", "1")
    st_s = sambamba_amd.view(path, b, format="sam", **kw)
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES")
    monkeypatch.delenv("SBX_SAM_PIECE_BYTES", raising=False)
    print("%s: text_bytes %d n_batches %d n_windows %d" % (tag, st_s["stream_bytes"], st_s["n_batches"], st_s["n_windows"]))
    assert filecmp.cmp(a, b, shallow=False)
    assert (st_r["n_windows"], st_r["window_bytes"], st_r["n_pack_launches"], st_r["ms_pack"]) == (0, 0, 0, 0.0)
    if streamed:
        # the text has no window: n_windows counts the pieces of text handed to the file, at least one per batch that selects
        assert st_s["window_bytes"] == int(piece or 64 << 20) and st_s["n_pack_launches"] == 0
        assert (st_s["n_windows"] >= 1) == (st_s["n_entries_out"] > 0)
    for k in ("n_records_in", "n_records_selected", "n_entries_out", "stream_bytes", "n_regions", "n_batches"):
        assert st_r[k] == st_s[k], k
    text = open(a, "rb").read()
    if want is not None:
        assert text == want
    return st_r, st_s, text


def expected_text(path, header=b"", **sel):
    stream = inflate(path)
    recs = ref.select(split_stream(stream)[3], **sel)
    return header + sam_ref.sam_text(recs, [n for n, _ in ref.refs_of(stream)])


def test_sam_several_batches_and_the_header(ties, tmp_path, monkeypatch):
    import sambamba_amd
    header = sambamba_amd.markdup_header_text(UNSORTED, "view -h").encode()
    _, st, _ = both_sam(monkeypatch, ties, tmp_path, want=expected_text(ties, header), with_header=True, command_line="view -h")
    assert st["n_batches"] >= 5 and st["n_windows"] >= st["n_batches"] - 1
    _, st, text = both_sam(monkeypatch, ties, tmp_path, tag="none", num_filter="2048", with_header=True, command_line="view -h", want=header)
    assert st["n_windows"] == 0 and st["n_entries_out"] == 0
    # a batch that selects nothing between two that do: the unmapped reads of ties lie all over the file; the whole file as one batch
    both_sam(monkeypatch, ties, tmp_path, tag="big", batch="100000000", want=expected_text(ties))


def test_sam_one_line_per_piece(ties, tmp_path, monkeypatch):
    _, st, _ = both_sam(monkeypatch, ties, tmp_path, piece="1", filter="unmapped", want=expected_text(ties, keep=_unmapped))
    assert st["n_windows"] == st["n_entries_out"] > 100


def test_sam_selections(ties, tmp_path, monkeypatch):
    refs = ref.refs_of(inflate(ties))
    both_sam(monkeypatch, ties, tmp_path, tag="s", subsample=0.5, seed=77, want=expected_text(ties, subsample=(0.5, 77)))
    both_sam(monkeypatch, ties, tmp_path, tag="nf", num_filter="/16", want=expected_text(ties, bits=(0, 16)))
    _, st, _ = both_sam(monkeypatch, ties, tmp_path, tag="c1", regions=["c1"], want=expected_text(ties, regions=[ref.parse_region("c1", refs)]))
    assert st["n_regions"] == 1
    both_sam(monkeypatch, ties, tmp_path, tag="star", regions=["*"], want=expected_text(ties, regions=["*"]))
    lines = ["c1\t49\t150", "c2\t0\t50000", "c1\t0\t200\tname", "chrNotThere\t0\t10"]
    bed = str(tmp_path / "sel.bed")
    open(bed, "w").write("".join(l + "\n" for l in lines))
    both_sam(monkeypatch, ties, tmp_path, tag="bed", bed=bed, filter="mapping_quality >= 30",
             want=expected_text(ties, keep=_mapq30, bed=ref.merged_bed(lines, refs)))
    # two listed regions: the resident path whatever the hook says
    regions = ["c2", "c1:1-200"]
    _, st, _ = both_sam(monkeypatch, ties, tmp_path, tag="two", regions=regions, streamed=False,
                        want=expected_text(ties, regions=[ref.parse_region(r, refs) for r in regions]))
    assert st["n_windows"] == 0 and st["window_bytes"] == 0


def test_sam_valid_only_and_the_indexed_pass(ordered, tmp_path, monkeypatch):
    recs = _tie_records(n=2500, seed=3)
    bad = bamgen.make_record(0, 100, "4M", "ACGT", 30, name="not@valid")
    recs.insert(1700, bad)
    path = str(tmp_path / "v.bam")
    bamgen.write_bam(path, REFS, recs, text=UNSORTED, block_size=BLOCK, write_index=False)
    _, st, _ = both_sam(monkeypatch, path, tmp_path, valid=True, want=expected_text(path, keep=lambda r: r != bad))
    assert st["n_records_selected"] == len(recs) - 1
    refs = ref.refs_of(inflate(ordered))
    region = "c1:10000-30000"
    st_r, st_s, _ = both_sam(monkeypatch, ordered, tmp_path, tag="ix", regions=[region], use_index=True, batch="9000",
                             want=expected_text(ordered, regions=[ref.parse_region(region, refs)]))
    assert st_s["blocks_read"] == st_r["blocks_read"] < st_r["blocks_in_file"] and st_s["n_batches"] >= 3


def test_sam_malformed_tag_in_a_later_batch(tmp_path, monkeypatch):
    """a selected record whose B tag runs past the record, in the third batch and later of a streamed run to a file: SBX_EFORMAT with
    the message of the resident path, and no output file although the text of the batches before it was written"""
    import sambamba_amd
    recs = [sam_cases.good_record(k) for k in range(1500)]
    recs[1400] = sam_cases.malformed_records()["b_count_past_end"]
    path = str(tmp_path / "bad.bam")
    info = bamgen.write_bam(path, sam_cases.REFS, recs, text=sam_cases.TEXT, block_size=BLOCK, write_index=False)
    assert info["records"][1400][3] > 3 * int(BATCH)              # (behind the third batch)
    monkeypatch.setenv("SBX_INDEX_BATCH_BYTES", BATCH)
    seen = []
    for hook in (None, "1"):
        if hook:
            monkeypatch.setenv("SBX_STREAM_WINDOW_BYTES", hook)
        out = str(tmp_path / "bad.sam")
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.view(path, out, format="sam")
        seen.append((ei.value.code, ei.value.msg))
        assert not os.path.exists(out)
    assert seen[0] == seen[1] and seen[0][0] == -3 and "(1 records" in seen[0][1]
    # not selected: no error on either path
    monkeypatch.delenv("SBX_STREAM_WINDOW_BYTES")
    want = sam_ref.sam_text([r for k, r in enumerate(recs) if k != 1400], sam_cases.REF_NAMES)
    bad = bytearray(recs[1400])
    struct.pack_into("<H", bad, 18, struct.unpack_from("<H", bad, 18)[0] | 0x200)
    recs[1400] = bytes(bad)
    bamgen.write_bam(path, sam_cases.REFS, recs, text=sam_cases.TEXT, block_size=BLOCK, write_index=False)
    both_sam(monkeypatch, path, tmp_path, tag="left_out", num_filter="/512", want=want)
