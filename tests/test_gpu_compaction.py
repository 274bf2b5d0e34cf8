"""File-order compaction at wave and workgroup edges.  sort -F (K9a), view -F to BAM (K12a / K12b) and markdup -r (K10's compact
kernels) all place the records they keep with one helper (wave_prims.hpp: ballot, popcount per wave through LDS, the waves in front,
the lanes below) behind a scan over the workgroups of 256.  The files here hold n records for the smallest n that cross one wave
(63, 64, 65), one workgroup (255, 256, 257) and two (513), and drop records in two patterns: every third one, and all but the last
lane of each wave.  Every output is compared byte for byte, inflated, with the Python restatements (sort_ref, view_ref, markdup_ref)."""
import struct

import pytest

from tests import bamgen
from tests import markdup_ref, sort_ref, view_ref
from tests.flagstat_ref import inflate

pytestmark = pytest.mark.gpu

REFS = [("c1", 100000)]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:100000\n"
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
PATTERNS = {"thirds": lambda i: i % 3 != 0, "wave_tails": lambda i: i % 64 == 63}
FILTER = "mapping_quality >= 30"


def _kept_by_filter(rec):
    return ((struct.unpack_from("<I", rec, 12)[0] >> 8) & 0xFF) >= 30


def records(n, pattern, file_index):
    """Record i is kept iff PATTERNS[pattern](i).  Kept: mapq 60, a position of its own, base quality 40.  Dropped: mapq 0, and a
    lower-scoring fragment at the position and strand of the first kept record, hence its duplicate (when there is a kept record)."""
    keep = PATTERNS[pattern]
    pos = lambda i: 100 + 3 * ((i * 37) % 1024)                 # distinct for i < 1024
    anchor = next((i for i in range(n) if keep(i)), 0)
    recs = []
    for i in range(n):
        name = "f%d_r%04d" % (file_index, i)
        if keep(i):
            recs.append(bamgen.make_record(0, pos(i), "10M", "ACGTACGTAC", 40, name=name, mapq=60, flag=0))
        else:
            recs.append(bamgen.make_record(0, pos(anchor), "10M", "ACGTACGTAC", 20, name=name, mapq=0, flag=0))
    return recs


def n_kept(n, pattern):
    return sum(1 for i in range(n) if PATTERNS[pattern](i))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """(n, pattern) -> (path, expected sort -F stream, expected view -F stream, expected markdup -r stream); computed once."""
    d = tmp_path_factory.mktemp("compaction")
    out = {}
    for k, (n, pattern) in enumerate((n, p) for n in SIZES for p in PATTERNS):
        path = str(d / ("%s_%d.bam" % (pattern, n)))
        bamgen.write_bam(path, REFS, records(n, pattern, k), text=TEXT, write_index=False)
        stream = inflate(path)
        out[(n, pattern)] = (path, sort_ref.expected_stream(stream, _kept_by_filter), view_ref.expected_stream(stream, "view", keep=_kept_by_filter),
                             markdup_ref.expected_stream(stream, True, "markdup"))
    return out


@pytest.mark.parametrize("pattern", sorted(PATTERNS))
@pytest.mark.parametrize("n", SIZES)
def test_kept_records_at_wave_and_workgroup_edges(files, n, pattern, tmp_path):
    import sambamba_amd
    path, want_sort, want_view, want_markdup = files[(n, pattern)]
    kept = n_kept(n, pattern)
    out = str(tmp_path / "sort.bam")
    st = sambamba_amd.sort_bam(path, out, filter=FILTER)
    assert (st["n_records_in"], st["n_records_out"]) == (n, kept)
    assert inflate(out) == want_sort
    out = str(tmp_path / "view.bam")
    st = sambamba_amd.view(path, out, filter=FILTER, command_line="view")
    assert (st["n_records_in"], st["n_entries_out"]) == (n, kept)
    assert inflate(out) == want_view
    out = str(tmp_path / "markdup.bam")
    st = sambamba_amd.markdup(path, out, remove_duplicates=True, command_line="markdup")
    # without a kept record the dropped ones are one group of fragments, and its best member stays
    assert (st["n_records_in"], st["n_records_out"]) == (n, kept if kept else 1)
    assert inflate(out) == want_markdup
