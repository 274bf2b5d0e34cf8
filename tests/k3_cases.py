"""Hand-placed inputs for K3 (`decode_accumulate`, sambamba_amd/csrc/depth.hip): every builder puts reads ON one of the kernels'
hard-coded limits instead of near it by chance.  Pure Python on tests/bamgen.py; tests/test_k3_cases_cpu.py checks that each
builder still has the property its docstring states, tests/test_gpu_k3_edges.py compares the device with the oracle on them.

Every builder returns (refs, records, read_groups) for `bamgen.write_bam(path, refs, records, read_groups=read_groups)`.
The records of a contig are in file order, positions never decrease.

Geometry the designs rely on: a tile is T = tile_positions(n_samples) reference positions (1024 / 512 / 256 for 1 / 2 / 3
samples), the records of a tile are a contiguous range [r_lo, r_hi) of the file's records, and wave w of the tile's workgroup
takes the batches of 64 records r_lo + 64 * (4 i + w).  A scenario that depends on what shares a batch is a record sequence of
period 64, so every window of 64 consecutive records holds one full period whatever r_lo is."""
import random

from tests import bamgen as bg

ALL_CODES = "=ACMGRSVTWYHKDBN"      # the 16 four-bit base codes
QUALS = (2, 12, 23, 37)             # both sides of MIN_BQ
MIN_BQ = 20
STACK_POS = 500                     # the stacked position of every contig of stacks() / stacks_deep()
STACK_DEPTH = 65535
FLAG_DUP, FLAG_QCFAIL = 0x400, 0x200


def tile_positions(n_samples):
    t = 1
    while t * 2 <= 1024 // n_samples:
        t *= 2
    return max(16, t)


def read_groups_for(n_samples):
    return [("g%d" % i, "s%d" % i) for i in range(n_samples)] if n_samples > 1 else []


class _Maker:
    """Records with random sequences (all 16 codes) and qualities, the read group cycling over the samples."""
    def __init__(self, seed, n_samples):
        self.rng = random.Random(seed)
        self.S = n_samples
        self.n = 0

    def rec(self, ref, pos, cigar, flag=0, seq=None, mapq=60):
        cig = bg.parse_cigar(cigar) if isinstance(cigar, str) else cigar
        l_seq = sum(n for op, n in cig if op in "MIS=X")
        if seq is None:
            seq = "".join(self.rng.choice(ALL_CODES) for _ in range(l_seq))
        qual = [self.rng.choice(QUALS) for _ in range(l_seq)]
        tags = bg.tag_z("RG", "g%d" % (self.n % self.S)) if self.S > 1 else b""
        self.n += 1
        return bg.make_record(ref, pos, cig, seq, qual, name="k%d" % self.n, flag=flag, mapq=mapq, tags=tags)


def _layered(cells, T, n_layers=4):
    """Places (offset, cigar, ref_len) cells end to end in n_layers layers over contigs of T positions, the read's first aligned
    base at a position with pos & 15 == offset: no position is covered by more than n_layers reads.
    Returns [(contig, pos, cigar)], sorted."""
    out = []
    cursor = [(0, 0)] * n_layers
    for i, (off, cigar, ln) in enumerate(cells):
        layer = i % n_layers
        contig, at = cursor[layer]
        pos = at + ((off - at) & 15)
        if pos + ln > T:
            contig, pos = contig + 1, off
        assert pos + ln <= T
        out.append((contig, pos, cigar))
        cursor[layer] = (contig, pos + ln)
    out.sort(key=lambda r: (r[0], r[1]))
    return out


SWEEP_LENGTHS = range(1, 34)
BLOCK_EDGE_LENGTHS = (160, 161, 162, 168, 169, 176, 177)
BLOCK_EDGE_OFFSETS = (0, 1, 15)
SWEEP_MAX_DEPTH = 4


def alignment_sweep(n_samples=1):
    """Single-run reads on every alignment the block routine of K3 distinguishes.  T = tile_positions(n_samples).

    * contigs `in<k>` (T positions, one tile each): a read `nM` or `1SnM` for every tile offset of the first base
      t0 & 15 in 0..15, first-base parity in {0, 1} (the leading 1S) and n in 1..33, and the block-count edges
      n in BLOCK_EDGE_LENGTHS at t0 & 15 in {0, 1, 15}, both parities (161 bases at offset 15 are 11 blocks, 162 are 12;
      176 at offset 0 are 11, 177 are 12; 160 / 161 is the fast-path limit of k_accumulate16, 168 a pass of k_accumulate).
      No position of these contigs is covered by more than SWEEP_MAX_DEPTH reads.
    * contig `edge` (one tile per border and one more): reads that cross a tile border b: they begin d positions before b and have m bases
      behind it, for d in 1..17, parity in {0, 1}, m in 1..33 (the clip at the tile's start moves the first query base through
      both parities and every byte offset; the clip at the tile's end cuts d bases at offset (T - d) & 15), and d in 18..33 with
      m in {1, 16, 17} (every cut length mod 16 at a tile's end).  SWEEP_MAX_DEPTH reads per border.
    * contig `steps` (one tile): one read across each quarter of the tile (the borders of the four waves' shares of the span
      integration) with nothing before the next one, a read that begins at position 0 and one that ends at T.
    * contig `full` (one tile): one read of T bases, from position 0 to T.
    Sequences use all 16 base codes."""
    T = tile_positions(n_samples)
    mk = _Maker(100 + n_samples, n_samples)
    cells = []
    for n in SWEEP_LENGTHS:
        for off in range(16):
            for par in (0, 1):
                cells.append((off, ("1S" if par else "") + "%dM" % n, n))
    for n in BLOCK_EDGE_LENGTHS:
        for off in BLOCK_EDGE_OFFSETS:
            for par in (0, 1):
                cells.append((off, ("1S" if par else "") + "%dM" % n, n))
    placed = _layered(cells, T, SWEEP_MAX_DEPTH)
    n_in = placed[-1][0] + 1
    refs = [("in%d" % k, T) for k in range(n_in)]
    records = [mk.rec(c, pos, cig) for c, pos, cig in placed]
    # tile borders
    crossing = [(d, par, m) for d in range(1, 18) for par in (0, 1) for m in SWEEP_LENGTHS]
    crossing += [(d, par, m) for d in range(18, 34) for par in (0, 1) for m in (1, 16, 17)]
    n_borders = (len(crossing) + SWEEP_MAX_DEPTH - 1) // SWEEP_MAX_DEPTH
    edge = len(refs)
    refs.append(("edge", (n_borders + 1) * T))
    rows = []
    for i, (d, par, m) in enumerate(crossing):
        b = (i // SWEEP_MAX_DEPTH + 1) * T
        rows.append((b - d, ("1S" if par else "") + "%dM" % (d + m)))
    rows.sort(key=lambda r: r[0])
    records += [mk.rec(edge, pos, cig) for pos, cig in rows]
    # span steps
    steps = len(refs)
    refs.append(("steps", T))
    h = T // 16
    rows = [(0, "%dM" % (h // 2))] + [(q * T // 4 - h, "%dM" % (2 * h)) for q in (1, 2, 3)] + [(T - h // 2, "%dM" % (h // 2))]
    records += [mk.rec(steps, pos, cig) for pos, cig in rows]
    refs.append(("full", T))
    records.append(mk.rec(steps + 1, 0, "%dM" % T))
    return refs, records, read_groups_for(n_samples)


# ---- the second stage's queues ---------------------------------------------------------------------------------------------
MDM, MNM, MIM, MIMIM = "7M3D9M", "6M4N8M", "9M2I8M", "5M1I6M2I7M"
OPS8 = "4S5M1I5M2D5M1I5M"           # 8 operations: 4 runs, 1 gap, walked by its lane
OPS9 = "4S5M1I5M2D5M1I5M3S"         # 9 operations: one more than a lane walks
SINGLE = "21M"


def _period(kind2, n_dropped=12):
    """64 CIGAR / flag pairs: the kind-2 reads spread evenly among single-run reads and reads the default filter drops."""
    fill = [(SINGLE, FLAG_DUP if i % 2 else FLAG_QCFAIL) for i in range(n_dropped)]
    fill += [(SINGLE if i % 3 else "2S19M", 0) for i in range(64 - len(kind2) - n_dropped)]
    random.Random(len(kind2)).shuffle(fill)
    out, k = [], 0
    for i in range(64):
        # Bresenham: kind-2 read k goes where i * len(kind2) / 64 steps
        if k < len(kind2) and (i * len(kind2)) // 64 >= k:
            out.append((kind2[k], 0))
            k += 1
        else:
            out.append(fill.pop())
    assert k == len(kind2) and not fill and len(out) == 64
    return out


PERIODS = {
    # name: (kind-2 reads of a period, run items, gap items, run blocks or None) per window of 64 records
    "a_full": ([MDM] * 4 + [MNM] * 4 + [MIM] * 3, 22, 8),
    "b_runs23": ([MDM] * 4 + [MNM] * 4 + [MIM] * 2 + [MIMIM] + [OPS9] * 2, 23, 8),
    "c_gaps9": ([MDM] * 5 + [MNM] * 4 + [MIM] * 2 + [OPS9] * 2, 22, 9),
    "f_ops8_9": ([OPS8] * 4 + [OPS9] * 4, 16, 4),
}
BIG = ["256M16D256M"] * 8 + ["256M1I256M"] * 3          # 22 runs of 256 bases, 8 gaps
BIG17 = BIG[:-1] + ["256M1I257M"]
NEAR_END = ["8M2I8M2I8M"] * 9 + ["10M4D10M"] * 4       # placed 12 positions before the tile's end
NEAR_END23 = ["8M2I8M2I8M"] * 9 + ["10M4D10M"] * 5


def queue_periods(n_samples=1):
    """One contig per design; the record sequence of every contig has period 64 and a multiple of 256 records, so every batch of
    64 descriptors holds exactly one period.  Run items are the runs of aligned bases, gap items the D / N runs, of the reads with
    a general CIGAR of at most 8 operations (what the lanes of k_accumulate16c walk), counted only where they touch the tile.

    * `a_full`: 22 run items and 8 gap items per 64 records: both queues full, no overflow.
    * `b_runs23`: 23 run items, 8 gap items: the run queue overflows alone.
    * `c_gaps9`: 9 gap items, 22 run items: the gap queue overflows alone.
    * `f_ops8_9`: CIGARs of 8 operations (queued) and of 9 (one read at a time) in one batch, no overflow; `b` and `c` carry
      two reads of 9 operations too, so an overflowing batch holds reads that were never queued.
    One sample only (runs of 256 bases need the 1024-position tile):
    * `d_blocks352`: 22 run items of exactly 16 blocks (256-base runs that begin at t0 & 15 == 0) and 8 gap items: 352 blocks.
    * `e_blocks353`: the same with one run of 257 bases: 22 items, 353 blocks: the block map overflows alone.
    * `g_outside`: every read begins 12 positions before the tile's end, on a contig of one tile: of the 35 runs of a period
      22 touch the first tile (with 4 gap items) and 22 the spare tile behind it (4 gap items).
    * `g_outside23`: the same with 23 run items in either tile (37 runs).
    The rest of each period are single-run reads and reads the default filter drops (duplicate, failed QC)."""
    T = tile_positions(n_samples)
    mk = _Maker(200 + n_samples, n_samples)
    refs, records = [], []
    n_rec = 512 if T == 1024 else 256

    def contig(name, period, pos_of):
        ref = len(refs)
        refs.append((name, T))
        for i in range(n_rec):
            cig, flag = period[i % 64]
            records.append(mk.rec(ref, pos_of(i), cig, flag=flag))

    for name in ("a_full", "b_runs23", "c_gaps9", "f_ops8_9"):
        contig(name, _period(PERIODS[name][0]), lambda i: 4 + (i * (T - 64)) // n_rec)
    if n_samples == 1:
        contig("d_blocks352", _period(BIG), lambda i: 16 * ((i * 30) // n_rec))
        contig("e_blocks353", _period(BIG17), lambda i: 16 * ((i * 30) // n_rec))
        contig("g_outside", _period(NEAR_END), lambda i: T - 12)
        contig("g_outside23", _period(NEAR_END23), lambda i: T - 12)
    return refs, records, read_groups_for(n_samples)


# ---- 2^16 records in a tile ------------------------------------------------------------------------------------------------
def stacks():
    """Four contigs of one tile (1024 positions, one sample).  On each, exactly STACK_DEPTH = 65,535 records -- one fewer than the
    limit of the 16-bit counters -- all cover STACK_POS, four of them longer reads so that the neighbouring positions are not empty:
    * `all_A`: base A there: the low half of the {A|C} dword is 0xFFFF beside an empty high half;
    * `all_C`: the high half of the same dword;
    * `all_DEL`: `1M1D1M`: DEL, the high half of {other|DEL}, and the compact word's depth, reach 65,535;
    * `all_SKIP`: `1M1N1M`: REFSKIP.
    No tile of this file has 2^16 records, so region / window runs keep compact counters."""
    mk = _Maker(300, 1)
    refs, records = [], []
    for name, base, cigar in (("all_A", "A", None), ("all_C", "C", None), ("all_DEL", None, "D"), ("all_SKIP", None, "N")):
        ref = len(refs)
        refs.append((name, 1024))
        records += _stack_records(mk, ref, STACK_DEPTH, base, cigar)
    return refs, records, []


def _stack_records(mk, ref, n, base, gap, at=STACK_POS):
    """n records that all cover position `at`: four longer reads, then n - 4 copies of one short read."""
    out = []
    if base:
        for k in (4, 3, 2, 1):          # longer reads: 9 bases, the stacked column is their base k
            seq = "".join(mk.rng.choice("GTN") for _ in range(9))
            out.append(mk.rec(ref, at - k, "9M", seq=seq[:k] + base + seq[k + 1:]))
        one = bg.make_record(ref, at, "1M", base, 30, name="s")
    else:
        for k in (4, 3, 2, 1):          # the gap of the longer reads lies on the stacked column too
            out.append(mk.rec(ref, at - k, "%dM1%s5M" % (k, gap)))
        one = bg.make_record(ref, at - 1, "1M1%s1M" % gap, "GT", [2, 37], name="s")
    return out + [one] * (n - len(out))


def stacks_deep():
    """Two contigs with a tile of exactly 65,536 records, which the 32-bit kernel takes (and which switches compact counters off):
    * `deep`: one tile, 65,536 records over STACK_POS (base A);
    * `deep_next_to_shallow`: two tiles, eight reads in the first and 65,536 records over 1024 + STACK_POS (base C) in the second."""
    mk = _Maker(301, 1)
    refs = [("deep", 1024), ("deep_next_to_shallow", 2048)]
    records = _stack_records(mk, 0, STACK_DEPTH + 1, "A", None)
    records += [mk.rec(1, 100 + 40 * i, "60M") for i in range(8)]
    records += _stack_records(mk, 1, STACK_DEPTH + 1, "C", None, at=1024 + STACK_POS)
    return refs, records, []


# ---- zero-length reference-consuming operations ----------------------------------------------------------------------------
ZERO_SHAPES = ("10M0M40M", "10M0N40M", "0D50M", "10M0D0D40M", "25=0=25=", "10M0D5I35M")
ZERO_PREFIX = "2S3M1I3M1D3M1I3M"        # 8 operations: what follows is the ninth
ZOO_SPACING = 16                        # one zoo read per 16 records: at most 4 per batch, so no batch overflows a queue


def zero_ninth(shape):
    """The shape with its first zero-length operation as the ninth operation of a longer CIGAR."""
    cig = bg.parse_cigar(shape)
    k = next(i for i, (op, n) in enumerate(cig) if n == 0)
    return ZERO_PREFIX + "".join("%d%s" % (n, op) for op, n in cig[k:])


def zero_length_zoo():
    """Zero-length reference-consuming operations (each still takes one pileup column in the reference): every shape of
    ZERO_SHAPES as it stands (at most 8 operations: walked by its lane) and with the zero-length operation as the ninth of a
    longer CIGAR (one read at a time), one such read per ZOO_SPACING records among single-run reads, so no batch overflows.
    * `zint`: in the interior of a tile;
    * `zedge` (two tiles): begun 11, 10 and 9 positions before the tile border at 1024 -- the column of the zero-length
      operation of the `10M0…` shapes is the last of the first tile, the first of the second, the second -- and at 1024."""
    mk = _Maker(400, 1)
    refs = [("zint", 1024), ("zedge", 2048)]
    records = []
    shapes = [s for z in ZERO_SHAPES for s in (z, zero_ninth(z))]

    def put(ref, pos, shape):
        records.append(mk.rec(ref, pos, shape))
        for i in range(ZOO_SPACING - 1):
            records.append(mk.rec(ref, pos, "30M" if i % 2 else "1S29M"))

    for i, s in enumerate(shapes):
        put(0, 40 + 70 * i, s)
    for pos in (1013, 1014, 1015, 1024):
        for s in shapes:
            put(1, pos, s)
    return refs, records, []
