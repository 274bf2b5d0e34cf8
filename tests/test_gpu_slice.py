"""`sambamba slice` on the device -- sbx_slice_bam: the edge runs, K18 (slice.hip) and the splice writer -- through the Python API and
the `sbx-slice` CLI, against the Python restatement of the definition (tests/slice_ref.py).  For every case the output inflates (zlib)
to exactly the expected stream, ends in the EOF block, holds no empty block that is not a copied one, and contains every block of
the input that lies wholly inside a region's stretch byte for byte and in order.  Files come from tests/bamgen.py with small blocks,
so that a few hundred records span dozens of blocks; indexes are built with sambamba_amd.build_index."""
import os
import struct
import subprocess

import pytest

from tests import bamgen
from tests.slice_ref import Bam, check_output, inflate_file, slice_ref
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

REFS = [("chr1", 200000), ("chr2", 100000), ("chr3", 50000), ("chr4", 50000)]
BLOCK = 600


def rec(ref, pos, cigar, name, flag=0):
    n = sum(k for op, k in bamgen.parse_cigar(cigar) if op in "MIS=X")
    return bamgen.make_record(ref, pos, cigar, "ACGT" * (n // 4) + "A" * (n % 4), 30, name=name, flag=flag)


def write(path, recs, cuts=None, refs=REFS):
    import sambamba_amd
    info = bamgen.write_bam(path, refs, recs, block_size=BLOCK, cuts=cuts, write_index=False)
    sambamba_amd.build_index(path, path + ".bai")
    return info


def main_records(unmapped=True):
    recs = [rec(0, 1000, "100M30000N100M", "spliced")]
    recs += [rec(0, 1000 + 40 * k, "50M", "a%04d" % k) for k in range(1, 3000)]          # chr1: 1040 .. 120960, one read per 40 positions
    recs += [rec(0, 130000, "", "nocigar", flag=0)]
    recs += [rec(0, 130000, "30M", "at130000"), rec(0, 130010, "30M", "b1"), rec(0, 150000, "50M", "far")]
    recs += [rec(1, 100 + 25 * k, "60M", "c%03d" % k) for k in range(300)]               # chr2: 100 .. 7575
    recs += [rec(3, 500 + 30 * k, "40M", "d%03d" % k) for k in range(100)]               # chr4 (chr3 has none)
    if unmapped:
        recs += [rec(-1, -1, "", "u%02d" % k, flag=4) for k in range(40)]
    return recs


@pytest.fixture(scope="module")
def main_bam(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("slice") / "main.bam")
    recs = main_records()
    info = bamgen.write_bam(path, REFS, recs, block_size=BLOCK, write_index=False)
    write(path, recs, cuts=[info["records"][k][3] for k in (200, 400, 600)])      # three records that begin a block
    return path, Bam(path)


def run(path, regions, tmp_path, tag, bed_lines=None, env=None):
    """the API (or, with env, the CLI) on `regions` / a BED file; the four properties; returns (stats, verbatim blocks, output path)"""
    import sambamba_amd
    out = str(tmp_path / (tag + ".bam"))
    bed = None
    if bed_lines is not None:
        bed = str(tmp_path / (tag + ".bed"))
        open(bed, "w").write("".join("%s\t%d\t%d\n" % l for l in bed_lines))
    st = None
    if env is None:
        st = sambamba_amd.slice_bam(path, out, regions=regions, bed=bed)
    else:
        args = ["-o", out] + (["-L", bed] if bed else []) + [path] + list(regions)
        r = subprocess.run([sambamba_amd.slice_cli_path()] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, **env))
        assert r.returncode == 0, r.stderr.decode()
    if bed_lines is not None:                       # the merged BED in (reference, start) order, as triples
        names = [n for n, _ in Bam(path).refs]
        want = sorted((names.index(c), b, e) for c, b, e in bed_lines if c in names)
    else:
        want = list(regions)
    n_verbatim = check_output(out, path, want)
    if st is not None:
        print("%s: %s" % (tag, st))
        assert st["blocks_copied"] == n_verbatim
    return st, n_verbatim, out


def region_at(bam, k0, k1, d0=0, d1=0):
    """chr1 region from the position of record k0 (+ d0) to that of record k1 (+ d1), 1-based inclusive text"""
    return "chr1:%d-%d" % (bam.recs[k0][2] + d0 + 1, bam.recs[k1][2] + d1)


def test_edges_against_block_boundaries(main_bam, tmp_path):
    path, bam = main_bam
    starts = {u: k for k, u in enumerate(bam.u[:-1])}
    on_start = [starts[o] for o in bam.block_start if o in starts and 100 < starts[o] < 1000]        # records that begin a block
    assert len(on_start) >= 3
    cut = [k for k in range(100, 1000) if any(bam.u[k] < o < bam.u[k + 1] for o in bam.block_start)]  # records cut by a boundary
    blk = lambda k: max(b for b in range(len(bam.blocks)) if bam.block_start[b] <= bam.u[k])
    k = next(k for k in range(100, 1000) if blk(k) == blk(k + 2) and bam.u[k] != bam.block_start[blk(k)])
    cases = {
        "one_block": region_at(bam, k, k + 2),                                  # a and b inside one block
        "a_on_start": region_at(bam, on_start[0], on_start[0] + 30, 0, -5),
        "b_on_start": region_at(bam, on_start[0] - 33, on_start[1]),
        "both_on_start": region_at(bam, on_start[0], on_start[2]),              # head and tail both empty
        "a_cut": region_at(bam, cut[0], cut[0] + 50),                           # the first record of the stretch straddles two blocks
        "b_cut": region_at(bam, cut[1] - 50, cut[2]),                           # ... and the first record behind it
    }
    for tag, region in cases.items():
        st, n_verbatim, _ = run(path, [region], tmp_path, tag)
        if tag == "one_block":
            assert n_verbatim == 0 and st["records_r1"] == 2                   # (50M every 40: one read reaches over beg, and the spliced one)
        if tag == "both_on_start":
            assert st["stream_bytes"] == bam.header_len + sum(len(bam.stream[bam.u[i]:bam.u[i + 1]]) for i in range(len(bam.recs))
                                                              if bam.recs[i][1] == 0 and bam.recs[i][2] < bam.recs[on_start[0]][2]
                                                              and bam.recs[i][2] + bam.recs[i][3] > bam.recs[on_start[0]][2])


def test_contigs_and_ends(main_bam, tmp_path):
    path, bam = main_bam
    for tag, regions in {
        "no_reads_here": ["chr1:160001-180000"],            # a contig with reads, none of them here
        "empty_contig": ["chr3"],
        "r1_only": ["chr1:1031-1035"],                      # beg inside the first reads, nothing starts in the region
        "r2_only": ["chr2:1-150"],                          # nothing in front of the contig's first read
        "whole_contig": ["chr2"],
        "to_the_end": ["chr2:5001"],
        "last_contig_then_unmapped": ["chr4:1001"],
        "unmapped": ["*"],
        "nocigar_at_beg": ["chr1:130001-130020"],
        "far_in_front": ["chr1:30001-30400"],               # the spliced read starts 29000 positions in front of beg
        "twice": ["chr1:2001-9000", "chr1:5001-12000"],     # two listed regions that overlap
        "out_of_order": ["chr4", "chr2:201-400", "chr1:150001-160000"],
    }.items():
        st, _, out = run(path, regions, tmp_path, tag)
        _, _, per = slice_ref(path, regions)
        if tag == "nocigar_at_beg":
            assert [r[36:36 + r[12] - 1] for r in per[0]][:2] == [b"nocigar", b"at130000"] and st["records_r1"] == 0
        if tag == "far_in_front":
            assert per[0][0][36:43] == b"spliced" and st["records_r1"] == 2
        if tag in ("empty_contig", "no_reads_here"):
            assert st["stream_bytes"] == bam.header_len and st["blocks_copied"] == 0


def test_last_contig_followed_by_nothing(tmp_path):
    path = str(tmp_path / "nounmapped.bam")
    write(path, main_records(unmapped=False))
    for tag, regions in {"last_whole": ["chr4"], "last_tail": ["chr4:2001"], "star": ["*"], "chr2_to_end": ["chr2:7001-100000"]}.items():
        run(path, regions, tmp_path, tag)


@pytest.mark.parametrize("n_r1", [63, 64, 65, 255, 256, 257, 1025])
def test_r1_at_the_wavefront_and_workgroup_limits(tmp_path, n_r1):
    recs = [rec(0, 100 + k, "20M", "p%03d" % k) for k in range(50)]
    recs += [rec(0, 5000, "200M", "r%04d" % k) for k in range(n_r1)]           # all of R1 over one position, spread over many blocks
    recs += [rec(0, 5100 + 10 * k, "20M", "q%03d" % k) for k in range(80)]
    path = str(tmp_path / "pile_in.bam")
    write(path, recs)
    st, _, _ = run(path, ["chr1:5101-5500"], tmp_path, "pile")
    assert st["records_r1"] == n_r1


@pytest.mark.parametrize("n_regions", [63, 64, 65, 257])
def test_many_regions_through_a_bed_file(main_bam, tmp_path, n_regions):
    path, bam = main_bam
    step = 45000 // n_regions                               # chr1 reads span 1040 .. 120960: every region's edges lie in different blocks
    assert step >= 160
    bed = [("chr1", 1500 + step * k, 1500 + step * k + step - 30) for k in range(n_regions)]
    bed = bed[::-1] + [("chrUn", 5, 10)]                    # (given unsorted; a contig the BAM lacks is dropped)
    st, _, _ = run(path, (), tmp_path, "bed%d" % n_regions, bed_lines=bed)
    assert st["n_regions"] == n_regions


def test_bed_whose_edge_runs_share_blocks_and_the_cli(main_bam, tmp_path):
    path, bam = main_bam
    bed = [("chr1", 2000 + 60 * k, 2000 + 60 * k + 20) for k in range(40)] + [("chr2", 200, 4000), ("chr4", 0, 50000)]
    _, _, a = run(path, (), tmp_path, "shared", bed_lines=bed)
    _, _, b = run(path, (), tmp_path, "shared_cli", bed_lines=bed, env={"SBX_TIMING": "1"})
    _, _, c = run(path, (), tmp_path, "shared_piece1", bed_lines=bed, env={"SBX_BGZF_PIECE_BLOCKS": "1"})
    assert open(a, "rb").read() == open(b, "rb").read() == open(c, "rb").read()
    regions = ["chr1:2001-30000", "chr2"]
    _, _, d = run(path, regions, tmp_path, "listed")
    _, _, e = run(path, regions, tmp_path, "listed_piece1", env={"SBX_BGZF_PIECE_BLOCKS": "1"})
    assert open(d, "rb").read() == open(e, "rb").read()
    # stdout
    import sambamba_amd
    r = subprocess.run([sambamba_amd.slice_cli_path(), path] + regions, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == open(d, "rb").read()


@pytest.mark.parametrize("name", ["issue_204", "issue225", "mate_overlaps_1_3M_4M", "issue_193"])
def test_golden_files(tmp_path, name):
    path = os.path.join(GOLDEN, name + ".bam")
    bam = Bam(path)
    mapped = [r for r in bam.recs if r[1] >= 0]
    regions = []
    if mapped:
        r, lo, hi = mapped[0][1], mapped[0][2], max(m[2] for m in mapped if m[1] == mapped[0][1])
        mid = (lo + hi) // 2
        ref_name = bam.refs[r][0]
        regions = [ref_name]
        if hi - lo > 4:
            regions += ["%s:%d-%d" % (ref_name, lo + 2, mid + 1), "%s:%d-%d" % (ref_name, mid + 1, hi + 1), "%s:%d" % (ref_name, mid)]
        last = mapped[-1][1]
        regions.append(bam.refs[last][0])
    for k, g in enumerate(regions):
        run(path, [g], tmp_path, "%s_%d" % (name, k))
    run(path, regions, tmp_path, name + "_all")
    run(path, ["*"], tmp_path, name + "_star")


# ---- the cost condition ----
def read_bai(path):
    d = open(path, "rb").read()
    n_ref = struct.unpack_from("<i", d, 4)[0]
    o, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", d, o)[0]
        o += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", d, o)
            o += 8
            bins[b] = [struct.unpack_from("<QQ", d, o + 16 * k) for k in range(n_chunk)]
            o += 16 * n_chunk
        n_intv = struct.unpack_from("<i", d, o)[0]
        o += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, d, o))))
        o += 8 * n_intv
    return refs


def blocks_the_index_names(bam, bai_ref, positions):
    """The blocks of the chunks of every bin that contains one of the positions, cut by the linear index at the first position -- what
    the index gives for them -- plus, per merged chunk, the one block that joining chunks a block apart may add."""
    bins, lin = bai_ref
    mo = lin[min(positions[0] >> 14, len(lin) - 1)] if lin else 0
    ids = set()
    for x in positions:
        ids |= {0, 1 + (x >> 26), 9 + (x >> 23), 73 + (x >> 20), 585 + (x >> 17), 4681 + (x >> 14)}
    coffs = [b[0] for b in bam.blocks]
    touched, n_chunks = set(), 0
    for b in ids:
        for beg, end in bins.get(b, []):
            if end <= mo:
                continue
            beg = max(beg, mo)
            n_chunks += 1
            for k, co in enumerate(coffs):
                if (beg >> 16) <= co and (co < (end >> 16) or (co == (end >> 16) and end & 0xFFFF)):
                    touched.add(k)
    return len(touched) + n_chunks


def test_cost_does_not_grow_with_the_region(main_bam, tmp_path):
    """A region of chr1 that spans more than 40 blocks: every block inside the stretch is copied, and what is inflated is bounded by
    what the .bai names for the two edge positions -- the chunks of the bins that contain them (with the block a join may add), one
    block per edge for the first record behind the edge's window, and the header's blocks -- whatever lies between the edges."""
    path, bam = main_bam
    beg, end = 3000, 115000
    st, n_verbatim, _ = run(path, ["chr1:%d-%d" % (beg + 1, end)], tmp_path, "cost")
    assert n_verbatim >= 40 and st["blocks_copied"] == n_verbatim
    header_blocks = sum(1 for o in bam.block_start[:-1] if o < bam.header_len)
    bound = blocks_the_index_names(bam, read_bai(path + ".bai")[0], [beg, end]) + 2 + header_blocks
    print("cost: blocks_inflated %d, bound %d, copied %d" % (st["blocks_inflated"], bound, n_verbatim))
    assert bound < n_verbatim / 2
    assert st["blocks_inflated"] <= bound


def test_same_records_as_view(main_bam, tmp_path):
    """On regions whose stretch holds no record without covered bases, slice and view select the same records."""
    import sambamba_amd
    path, bam = main_bam
    for k, region in enumerate(["chr1:2001-9000", "chr2:1001-3000", "chr4"]):
        _, _, out = run(path, [region], tmp_path, "x%d" % k)
        view_out = str(tmp_path / ("v%d.bam" % k))
        sambamba_amd.view(path, view_out, regions=[region])
        got, want = Bam(out), Bam(view_out)
        assert got.stream[got.header_len:] == want.stream[want.header_len:] and len(got.recs) > 0


# ---- refusals ----
def test_refusals_leave_no_output(main_bam, tmp_path):
    import shutil
    import sambamba_amd
    path, _ = main_bam
    out = str(tmp_path / "refused.bam")

    def refused(code, word, *args, **kw):
        with pytest.raises(sambamba_amd.SbxError) as ei:
            sambamba_amd.slice_bam(*args, **kw)
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
        assert not os.path.exists(out)

    bare = str(tmp_path / "bare.bam")
    shutil.copy(path, bare)
    refused(-7, "index", bare, out, regions=["chr1"])                          # SBX_ENOINDEX
    refused(-1, "chrNope", path, out, regions=["chr1:1-10", "chrNope:5-9"])
    refused(-1, "*", path, out, regions=["*", "chr1"])
    refused(-1, "empty", path, out, regions=["chr1:300-200"])
    refused(-1, "Must provide", path, out)
    with pytest.raises(sambamba_amd.SbxError) as ei:
        sambamba_amd.slice_bam(path, path, regions=["chr1"])
    assert ei.value.code == -1 and "overwrite" in str(ei.value)
    assert inflate_file(path)[0] == main_bam[1].stream
