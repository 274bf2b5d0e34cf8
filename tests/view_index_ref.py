"""Which BGZF blocks an indexed `view` reads, restated in Python from the BAI format (SAM specification, section 5.2) and the chunk
query of the reference (BioD bio/std/hts/bam/randomaccessmanager.d:247-294): per contig the regions are merged, the bins of every
merged region collected (bin 0 always), the chunks of those bins cut at the linear-index entry of the first region's window, sorted
and merged; every chunk becomes a run of blocks, and runs that share a block or lie at most one block apart are joined.  The region
`*` adds the blocks from the first record without a reference -- the highest chunk end of the index -- to the end of the stream.
Test harness only: tests/test_gpu_view_index.py compares sbx_view_index_stats with it."""
import struct

from tests.slice_ref import read_blocks

MAX_BIN = 37449         # ids below it are bins of the UCSC scheme; 37450 is the pseudo-bin with the counts


def read_bai(path):
    """[(bins: {id: [(beg, end)]}, linear index)] per reference"""
    d = open(path, "rb").read()
    assert d[:4] == b"BAI\1"
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


def region_bins(beg, end):
    """the bins that may hold a record overlapping [beg, end)"""
    end -= 1
    ids = {0}
    for first, shift in ((1, 26), (9, 23), (73, 20), (585, 17), (4681, 14)):
        ids |= set(range(first + (beg >> shift), first + (end >> shift) + 1))
    return {b for b in ids if b < MAX_BIN}


def merge_regions(regions):
    """{ref_id: [(start, end)]} sorted by start, overlapping and touching ones merged"""
    by = {}
    for r, s, e in sorted(regions):
        g = by.setdefault(r, [])
        if g and g[-1][1] >= s:
            g[-1] = (g[-1][0], max(g[-1][1], e))
        else:
            g.append((s, e))
    return by


def group_chunks(bai_ref, group):
    bins, lin = bai_ref
    ids = set()
    for s, e in group:
        ids |= region_bins(s, e)
    mo = lin[min(group[0][0] >> 14, len(lin) - 1)] if lin else 0
    chunks = sorted((max(beg, mo), end) for b in ids for beg, end in bins.get(b, []) if end > mo)
    merged = []
    for beg, end in chunks:
        if merged and merged[-1][1] >= beg:
            merged[-1][1] = max(merged[-1][1], end)
        else:
            merged.append([beg, end])
    return merged


class Layout:
    """the block table of a BAM: file offset and inflated offset of every block that holds bytes"""
    def __init__(self, path):
        _, blocks = read_blocks(path)
        self.coff = [b[0] for b in blocks]
        self.off = [0]
        for b in blocks:
            self.off.append(self.off[-1] + len(b[2]))
        self.total = self.off[-1]
        stream = b"".join(b[2] for b in blocks)
        l_text = struct.unpack_from("<i", stream, 4)[0]
        o = 8 + l_text
        n_ref = struct.unpack_from("<i", stream, o)[0]
        o += 4
        for _ in range(n_ref):
            o += 8 + struct.unpack_from("<i", stream, o)[0]
        self.first_record = o

    def stream_offset(self, v):
        co, uo = v >> 16, v & 0xFFFF
        if co not in self.coff:
            assert co > self.coff[-1]
            return self.total
        return self.off[self.coff.index(co)] + uo

    def block_of(self, u):
        return max(k for k in range(len(self.coff)) if self.off[k] <= u)


def runs_read(path, regions, bai_path=None):
    """regions: "*" or (ref_id, start, end).  The joined runs as [first block, end block) pairs."""
    lay = Layout(path)
    bai = read_bai(bai_path or path + ".bai")
    runs = []
    for r, group in merge_regions([g for g in regions if g != "*"]).items():
        if r >= len(bai):
            continue
        for beg, end in group_chunks(bai[r], group):
            if beg >= end:
                continue
            ub, ue = max(lay.stream_offset(beg), lay.first_record), min(lay.stream_offset(end), lay.total)
            if ub >= ue:
                continue
            b0 = lay.block_of(ub)
            be = lay.block_of(ue - 1)           # the block of the chunk's last byte
            runs.append((ub, b0, be + 1))
    if "*" in regions:
        ends = [end for bins, _ in bai for b, chunks in bins.items() if b < MAX_BIN for beg, end in chunks if beg < end]
        u = max(lay.stream_offset(max(ends)), lay.first_record) if ends else lay.first_record
        if u < lay.total:
            runs.append((u, lay.block_of(u), len(lay.coff)))
    joined = []
    for _, b0, b1 in sorted(runs):
        if joined and b0 <= joined[-1][1] + 1:
            joined[-1][1] = max(joined[-1][1], b1)
        else:
            joined.append([b0, b1])
    return [tuple(j) for j in joined]


def blocks_read(path, regions, bai_path=None):
    """the set of file blocks (indices into the blocks that hold bytes) the call reads"""
    return {b for b0, b1 in runs_read(path, regions, bai_path) for b in range(b0, b1)}
