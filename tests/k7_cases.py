"""Hand-placed inputs for K7 (`--fix-mate-overlaps`, sambamba_amd/csrc/mates.hip): every builder puts records ON one of the kernels'
hard-coded limits instead of near it by chance.  Pure Python on tests/bamgen.py; tests/test_k7_cases_cpu.py checks that each
builder still has the property its docstring states, tests/test_gpu_k7_edges.py compares the device with the oracle on them.

Every builder returns (refs, records, read_groups) for `bamgen.write_bam(path, refs, records, read_groups=read_groups)`; the
builders of refused inputs return {name: (refs, records, read_groups)}.  The records are in file order, which is the order of the
record indices on the device: (contig, position), then the order in which the builder made them.

Geometry the designs rely on: a tile is T = tile_positions(n_samples) reference positions; phase 1 of k_accumulate_mates takes a
read whose alignment is one run of M/=/X that lies inside its sequence, whose mate (if it has one) is of the same kind, and whose
part inside the tile touches at most 11 aligned blocks of 16 positions; every other record of the tile goes to the per-position
path through a list of 382 u16 indices.  k_find_mates_join: workgroup g owns the records [256 g, 256 g + 256) and stages the window
[256 g, 256 g + 1024) in LDS."""
import random

from tests import bamgen as bg
from tests.k3_cases import ALL_CODES, MIN_BQ, QUALS, _layered, read_groups_for, tile_positions  # noqa: F401  (MIN_BQ, QUALS: for the tests)

MAX_PAIRS = 4                       # pairs over one column in the sweep designs (A - C)
WORK_CAP = 382                      # kMateWorkCap
FAST_BLOCKS = 11
JOIN_WINDOW, JOIN_GROUP = 1024, 256


def fnv1a(name):
    h = 14695981039346656037
    for c in name.encode():
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


class _Maker:
    """Records with random sequences (all 16 codes) and qualities from QUALS; kept as (contig, position, serial, bytes)."""
    def __init__(self, seed, n_samples=1):
        self.rng = random.Random(seed)
        self.S = n_samples
        self.n = 0
        self.rows = []

    def name(self):
        self.n += 1
        return "p%d" % self.n

    def rec(self, ref, pos, cigar, name=None, group=None, mapq=60, flag=0, quals=None, l_seq=None):
        cig = bg.parse_cigar(cigar) if isinstance(cigar, str) else cigar
        if l_seq is None:
            l_seq = sum(n for op, n in cig if op in "MIS=X")
        seq = "".join(self.rng.choice(ALL_CODES) for _ in range(l_seq))
        qual = [self.rng.choice(quals or QUALS) for _ in range(l_seq)]
        if name is None:
            name = self.name()
        if group is None:
            group = self.n % self.S
        tags = bg.tag_z("RG", "g%d" % group) if self.S > 1 else b""
        self.rows.append((ref, pos, len(self.rows), bg.make_record(ref, pos, cig, seq, qual, name=name, flag=flag, mapq=mapq, tags=tags)))
        return len(self.rows) - 1

    def pair(self, ref, pos_a, cig_a, pos_b, cig_b, mapq=(60, 60), quals=None):
        """Two records of one name and one sample; the first one made comes first in the file when the positions are equal."""
        name = self.name()
        group = self.n % self.S
        self.rec(ref, pos_a, cig_a, name, group, mapq[0], quals=quals)
        self.rec(ref, pos_b, cig_b, name, group, mapq[1], quals=quals)

    def records(self):
        return [b for _, _, _, b in sorted(self.rows)]


def _m(n, parity=0):
    return ("1S" if parity else "") + "%dM" % n


# ---- A: phase 1, the aligned blocks of 16 positions ------------------------------------------------------------------------
SWEEP_STARTS = range(18)            # B begins d positions behind A
SWEEP_LENGTHS = range(1, 34)
BLOCK_EDGE_LENGTHS = (160, 161, 162, 176, 177)
BLOCK_EDGE_OFFSETS = (0, 1, 15)
EXTREME_QUALS = (0, 255)


def pair_sweep(n_samples=1):
    """Pairs of single-run reads (`nM` or `1SnM`) on every alignment phase 1 of k_accumulate_mates distinguishes, on contigs
    `in<k>` of one tile (T positions) each, at most MAX_PAIRS pairs over any column.  A is the mate that comes first in the file,
    B begins d positions behind it; both mates of a pair share a sample, the samples cycle over the pairs.

    * grid: A's first base at every tile offset t0 & 15 in 0..15, d in 0..17, both first-base parities of A and of B
      independently; A's length runs through d + 1..33 (the mates overlap), B's through 1..33.  At d = 0 the file order alone
      decides who is the second mate.
    * ends: for every t0 & 15 and every residue e, a pair whose overlap ends at a tile offset with residue e (B inside A, two
      positions behind A's start): the masks `ok0` / `ok1` at 0, 1, 15, 16, and overlaps wholly inside one block.
    * shapes: identical spans, A inside B (same start, B longer), B inside A, B beginning at A's end (abutting: no pair) and at
      A's last base (one shared column), at t0 & 15 in {0, 1, 7, 15} and lengths {1, 16, 17, 33}.
    * blocks: a run of n in BLOCK_EDGE_LENGTHS bases at t0 & 15 in BLOCK_EDGE_OFFSETS -- 161 bases at offset 15 and 176 at offset
      0 are 11 blocks (phase 1), 162 and 177 are 12 (per-position path) -- as A with a short B inside it, as B behind a short A,
      and as both mates with the same start: 176 with 177, 161 with 162 at offset 15, either one first -- one mate decided by the
      arithmetic of phase 1, the other by `state_at`, at the same columns.
    * extremes: pairs with the qualities 0 and 255 only, d in 0..3: the ends of `(qb - qa - tie) >> 31`."""
    T = tile_positions(n_samples)
    mk = _Maker(700 + n_samples, n_samples)
    cells = []      # (A's tile offset & 15, (d, cigar A, cigar B, qualities), length of the cell)

    def cell(off, d, cig_a, n_a, cig_b, n_b, quals=None):
        cells.append((off, (d, cig_a, cig_b, quals), max(n_a, d + n_b)))

    i = 0
    for off in range(16):
        for d in SWEEP_STARTS:
            for pa in (0, 1):
                for pb in (0, 1):
                    n_a = d + 1 + (i * 7) % (33 - d)
                    n_b = 1 + (i * 5 + off) % 33
                    cell(off, d, _m(n_a, pa), n_a, _m(n_b, pb), n_b)
                    i += 1
    for off in range(16):
        for e in range(16):
            n_b = ((e - off - 2 - 1) & 15) + 1          # 1..16: B = [off + 2, off + 2 + n_b) ends at residue e, inside A's 20 bases
            cell(off, 2, _m(20, e & 1), 20, _m(n_b, (e >> 1) & 1), n_b)
    for off in (0, 1, 7, 15):
        for n in (1, 16, 17, 33):
            for par in (0, 1):
                cell(off, 0, _m(n, par), n, _m(n, 1 - par), n)                      # identical spans
                cell(off, 0, _m(n, par), n, _m(n + 5, par), n + 5)                  # A inside B
                cell(off, 1, _m(n + 7, par), n + 7, _m(n, par), n)                  # B inside A
                cell(off, n, _m(n, par), n, _m(n, par), n)                          # abutting
                if n > 1:
                    cell(off, n - 1, _m(n, par), n, _m(n, 1 - par), n)              # one shared column
    for n in BLOCK_EDGE_LENGTHS:
        for off in BLOCK_EDGE_OFFSETS:
            for par in (0, 1):
                cell(off, 5, _m(n, par), n, _m(30, par), 30)                        # the long run is A
                cell((off - 5) & 15, 5, _m(30, par), 30, _m(n, par), n)             # the long run is B
    for off, n11, n12 in ((0, 176, 177), (15, 161, 162)):
        for par in (0, 1):
            cell(off, 0, _m(n11, par), n11, _m(n12, 1 - par), n12)
            cell(off, 0, _m(n12, par), n12, _m(n11, par), n11)
    for off in (0, 9, 15):
        for d in range(4):
            cell(off, d, _m(20, d & 1), 20, _m(20, off & 1), 20, EXTREME_QUALS)
    placed = _layered(cells, T, MAX_PAIRS)
    refs = [("in%d" % k, T) for k in range(placed[-1][0] + 1)]
    for contig, pos, (d, cig_a, cig_b, quals) in placed:
        mk.pair(contig, pos, cig_a, pos + d, cig_b, quals=quals)
    return refs, mk.records(), read_groups_for(n_samples)


# ---- B: tile borders -------------------------------------------------------------------------------------------------------
BORDER_BEFORE = range(1, 18)        # A begins d positions before the border
BORDER_BEHIND = (1, 15, 16, 17, 33)   # and has m bases behind it
BORDER_WAYS = ("before", "spans", "behind", "b_first", "ends_at")
A_FIRST, A_SECOND = (60, 59), (59, 60)      # on `edge` A has mapping quality 60, B 59 (no D / N there: it decides nothing)


def pair_borders(n_samples=1):
    """Pairs of single-run reads around tile borders, at most MAX_PAIRS pairs per border.  T = tile_positions(n_samples).

    * contig `edge`: A begins d in 1..17 positions before a border b and has m in BORDER_BEHIND bases behind it; B lies
      `before` (same start as A, ends before b -- at b when d = 1: the overlap is wholly before the border), `spans` (begins before b, ends
      behind it), `behind` (begins at or behind b: the overlap is wholly behind the border, and in that tile A is a mate that
      began in the tile before), `b_first` (B comes first in the file, beginning up to 9 positions before A), `ends_at` (the
      overlap ends exactly at b, tile offset T).  First-base parities cycle.
    * contigs `far<k>` (3 T): B begins 3 positions before the border T and ends inside A, which begins d in {1, 16, 17} before
      the border 2 T: in A's tile, `ts - b.pos` of `b_q0` is positive and B began in the tile before.
    * contig `last` (T + T / 2): a pair across the border T and a pair that ends at the contig's end, in its last, half tile.
    * contig `steps` (one tile): a pair across each quarter of the tile (the borders of the four waves' shares of the span
      integration) with nothing before the next one, a pair that begins at position 0 and one that ends at T."""
    T = tile_positions(n_samples)
    mk = _Maker(710 + n_samples, n_samples)
    cases = [(d, m, way) for d in BORDER_BEFORE for m in BORDER_BEHIND for way in BORDER_WAYS]
    n_borders = (len(cases) + MAX_PAIRS - 1) // MAX_PAIRS
    refs = [("edge", (n_borders + 1) * T)]
    for i, (d, m, way) in enumerate(cases):
        b = (i // MAX_PAIRS + 1) * T
        pa, pb = i & 1, (i >> 1) & 1
        a_pos, a = b - d, _m(d + m, pa)
        if way == "before":
            n = max(1, d - 1 - i % 3)
            mk.pair(0, a_pos, a, a_pos, _m(n, pb), A_FIRST)
        elif way == "spans":
            x = min(d - 1, i % 5)
            mk.pair(0, a_pos, a, a_pos + x, _m(d - x + 1 + i % 20, pb), A_FIRST)
        elif way == "behind":
            j = i % m
            mk.pair(0, a_pos, a, b + j, _m(1 + i % 33, pb), A_FIRST)
        elif way == "b_first":
            e = 1 + i % 9
            mk.pair(0, a_pos - e, _m(e + 1 + i % (d + m), pb), a_pos, a, A_SECOND)
        else:
            mk.pair(0, a_pos, a, a_pos + (d - 1) // 2, _m(d - (d - 1) // 2, pb), A_FIRST)
    for d in (1, 16, 17):
        for m in (1, 17):
            for x in (1, d, d + m):
                ref = len(refs)
                refs.append(("far%d" % (ref - 1), 3 * T))
                mk.pair(ref, T - 3, _m(T + 3 - d + x, ref & 1), 2 * T - d, _m(d + m, m & 1))
    ref = len(refs)
    refs.append(("last", T + T // 2))
    mk.pair(ref, T - 9, _m(20), T - 4, _m(21, 1))
    mk.pair(ref, T + T // 2 - 30, _m(30, 1), T + T // 2 - 12, _m(12))
    ref = len(refs)
    refs.append(("steps", T))
    h = T // 16
    mk.pair(ref, 0, _m(h // 2), 0, _m(h // 2 - 1, 1))
    for q in (1, 2, 3):
        mk.pair(ref, q * T // 4 - h, _m(2 * h), q * T // 4 - 1, _m(h, 1))
    mk.pair(ref, T - h // 2, _m(h // 2, 1), T - h // 2 + 1, _m(h // 2 - 1))
    return refs, mk.records(), read_groups_for(n_samples)


# ---- C: the per-position path and its rule ---------------------------------------------------------------------------------
KIND_SHAPES = ("10M2I10M", "10M3D10M", "10M5N10M", "4S20M", "20M4S", "3H20M", "20M3H", "10M2P10M", "10M0D10M", "10M0N10M", "10M0M10M")
KIND_MAPQ = ((50, 20), (20, 50), (30, 30))      # higher on the first mate, on the second, equal: the later record wins
KIND_STARTS = (0, 3, 8, 12)
KIND_SPACING = 64


def pair_kinds():
    """One contig, one sample, one pair per KIND_SPACING positions: a single-run `24M` read and a read of every shape of
    KIND_SHAPES (insertion, deletion, skip, soft and hard clips at either end, padding, zero-length D / N / M), the single-run
    read first and second in the file, the second mate KIND_STARTS positions behind the first (12: the first mate's D / N lies
    on the second one's first bases), mapping qualities KIND_MAPQ.  Then D against N: `10M4D10M` and `8M6N10M` two positions
    apart, so that D-vs-base, N-vs-base and D-vs-N columns all occur, under the same three mapping qualities."""
    mk = _Maker(720)
    at = KIND_SPACING
    for shape in KIND_SHAPES:
        for mapq in KIND_MAPQ:
            for d in KIND_STARTS:
                mk.pair(0, at, shape, at + d, "24M", mapq)
                at += KIND_SPACING
                mk.pair(0, at, "24M", at + d, shape, mapq)
                at += KIND_SPACING
    for mapq in KIND_MAPQ:
        mk.pair(0, at, "10M4D10M", at + 2, "8M6N10M", mapq)
        at += KIND_SPACING
    return [("kinds", at + KIND_SPACING)], mk.records(), []


def short_sequence():
    """A pair whose first mate is `20M` without a stored sequence (SEQ `*`, l_seq = 0, so q_start + span > l_seq: `single_run_ok`
    is false for a record K2 calls single-run), next to an ordinary pair.  The reference reads such a record's bases from whatever
    follows its empty sequence, so there is no oracle for it: the two paths of k_accumulate_mates are compared with each other."""
    mk = _Maker(725)
    name = mk.name()
    mk.rec(0, 100, "20M", name, l_seq=0)
    mk.rec(0, 105, "20M", name)
    mk.pair(0, 200, "20M", 205, "20M")
    return [("short", 1024)], mk.records(), []


# ---- D: the list of the per-position path ----------------------------------------------------------------------------------
LISTED = "5M1D5M"


def work_list():
    """One contig of 3 T = 3072 positions, one sample.  Tile 0 holds exactly WORK_CAP = 382 records that phase 1 leaves to the
    per-position path, tile 2 exactly 383 (the list overflows; phase 2 walks all records of the tile and repeats the eligibility
    test), tile 1 none.  The listed records are short `5M1D5M` reads alone, pairs of them (each other's mates: 91 pairs per tile)
    and pairs of one with a single-run `8M` read (listed for its mate's sake: 50 pairs); 210 pairs of `6M` reads that phase 1
    takes lie between them, 4 more in tile 1.
    The oracle's counters of this file take under 0.01 s (measured on a CPU; 1,613 records of at most 11 positions)."""
    T = 1024
    mk = _Maker(730)
    for tile, n_solo in ((0, 100), (2, 101)):
        units = ["solo"] * n_solo + ["both"] * 91 + ["mixed"] * 50 + ["fast"] * 210
        mk.rng.shuffle(units)
        for i, u in enumerate(units):
            pos = tile * T + 2 + (i * (T - 24)) // len(units)
            if u == "solo":
                mk.rec(0, pos, LISTED)
            elif u == "both":
                mk.pair(0, pos, LISTED, pos + 3, LISTED, mapq=(20 + i % 3, 21))
            elif u == "mixed":
                mk.pair(0, pos, LISTED if i & 1 else "8M", pos + 2, "8M" if i & 1 else LISTED, mapq=(20 + i % 3, 21))
            else:
                mk.pair(0, pos, "6M", pos + 3 - i % 4, "6M")
    for k in range(4):
        mk.pair(0, T + 100 + 200 * k, "6M", T + 103 + 200 * k, "6M")
    return [("list", 3 * T)], mk.records(), []


# ---- E: u16 record indices -------------------------------------------------------------------------------------------------
INDEX_PAIRS, INDEX_GAPPED = 300, 6


def index_limit(n):
    """One contig of exactly T = 1024 positions (one sample, one tile) with exactly n admitted records: n = 65,535 is the most
    the list's u16 indices address (`r_hi - r_lo > 0xFFFF` is false), n = 65,536 sends the tile to the walk over all records.
    Most records are `1M` reads with names of their own, 63 or 64 per position; INDEX_PAIRS = 300 pairs of `2M` reads that
    overlap in one or both columns lie among them, and INDEX_GAPPED = 6 `1M1D1M` reads, three of them the last records of the
    tile: with n = 65,535 the listed indices reach 65,534.
    The oracle's counters of either file take 0.02 s (measured on a CPU; reads of 1 to 3 positions keep its per-column sort at
    about 70 entries); building the records and writing the BAM takes 1.3 s."""
    T = 1024
    mk = _Maker(740 + (n & 1))
    n_fill = n - 2 * INDEX_PAIRS - INDEX_GAPPED
    for k in range(n_fill):
        mk.rec(0, (k * (T - 2)) // n_fill, "1M")
    for k in range(INDEX_PAIRS):
        mk.pair(0, 3 * k, "2M", 3 * k + (k & 1), "2M")
    for pos in (200, 500, 800):
        mk.rec(0, pos, "1M1D1M")
    for _ in range(3):
        mk.rec(0, T - 3, "1M1D1M")
    return [("tile", T)], mk.records(), []


# ---- F: the join's window --------------------------------------------------------------------------------------------------
JOIN_LANES = (0, 1, 127, 255)                   # A's index in its workgroup
JOIN_MATE_AT = (1023, 1024, 1025, 3000)         # the mate's index in A's window: the last in LDS, the first in global memory, ...
HALF_COLLISION = ("m93239", "m131074")          # FNV-1a hashes that agree in their low 32 bits (found by a search over m0..m399999)
CHAIN_NAME, CHAIN_LENGTH = "same", 300
A_POS, A_LEN = 300, 200


def join_window():
    """k_find_mates_join.  The record index on the device is the index in the file; the builder counts its own records.  On
    every contig `w<w>_t<t>` a `200M` read A is record t of its workgroup (index % 256 == t, t in JOIN_LANES) and its mate is
    record w of the window that begins at the workgroup's first record (w in JOIN_MATE_AT); the records between them are `1M`
    reads with names of their own that begin inside A's span, more of them follow the mate, inside A's span and behind it.
    Further contigs:
    * `next_ref`: A's window ends on the next contig (its last entry is a record of `filtered_last`), the mate lies before that;
    * `filtered_last`: entry 1023 of A's window is a record the default filter drops (mapq 0), the mate is entry 1100;
    * `dup_a`, `dup_b`: the last record of `dup_a` and the first two of `dup_b` have one name and the same coordinates: the
      two of `dup_b` pair, the one of `dup_a` pairs with neither;
    * `collide`: HALF_COLLISION -- two names whose hashes agree in the half the table is keyed by and differ in the other --
      each with its mate, all four records overlapping;
    * `chain`: CHAIN_LENGTH = 300 `1M` records of ONE name on 300 positions of their own (one probe chain of equal keys, no
      two overlap) and an overlapping pair of another name among them;
    * `file_end`: the file ends inside A's window and the mate is its last record."""
    mk = _Maker(750)
    refs = []

    def contig(name, length=1024):
        refs.append((name, length))
        return len(refs) - 1

    def fill(ref, pos, mapq=60):
        mk.rec(ref, pos, "1M", mapq=mapq)

    def scenario(name, t, w, filtered_at=None, after=40):
        ref = contig(name)
        k = 0
        while len(mk.rows) % JOIN_GROUP != t:
            fill(ref, 10 + k // 4)
            k += 1
        base = len(mk.rows) - t
        nm = mk.name()
        mk.rec(ref, A_POS, "%dM" % A_LEN, nm, 0)
        n_fill = base + w - len(mk.rows)
        for k in range(n_fill):
            fill(ref, A_POS + (k * 140) // n_fill, mapq=0 if len(mk.rows) - base == filtered_at else 60)
        assert len(mk.rows) - base == w
        mk.rec(ref, A_POS + 140, "80M", nm, 0)
        for k in range(after):
            fill(ref, A_POS + 140 + (k * 80) // after)      # the last ones lie behind A's end
        return ref

    for w in JOIN_MATE_AT:
        for t in JOIN_LANES:
            scenario("w%d_t%d" % (w, t), t, w)
    scenario("next_ref", 5, 505, after=100)
    scenario("filtered_last", 0, 1100, filtered_at=1023)
    ref = contig("dup_a")
    fill(ref, 50)
    mk.rec(ref, 100, "50M", "dup", 0)
    ref = contig("dup_b")
    mk.rec(ref, 100, "50M", "dup", 0)
    mk.rec(ref, 100, "50M", "dup", 0)
    fill(ref, 120)
    ref = contig("collide")
    for k, nm in enumerate(HALF_COLLISION * 2):
        mk.rec(ref, 100 + 10 * k, "60M", nm, 0)
    ref = contig("chain")
    other = mk.name()
    for pos in range(CHAIN_LENGTH):
        mk.rec(ref, pos, "1M", CHAIN_NAME, 0)
        if pos in (100, 120):
            mk.rec(ref, pos, "40M", other, 0)
    ref = contig("file_end")
    k = 0
    while len(mk.rows) % JOIN_GROUP != 3:
        fill(ref, 10 + k // 4)
        k += 1
    nm = mk.name()
    mk.rec(ref, A_POS, "%dM" % A_LEN, nm, 0)
    for k in range(400):
        fill(ref, A_POS + (k * 140) // 400)
    mk.rec(ref, A_POS + 140, "80M", nm, 0)
    rows = mk.rows
    assert rows == sorted(rows)         # made in file order: the indices counted above are the file's
    return refs, mk.records(), []


# ---- G: partner lists ------------------------------------------------------------------------------------------------------
GROUP_SPACING = 400
# (name, [(offset from the group's place, bases)] in the order made); the longest record of a group is A
PARTNER_GROUPS = (
    ("nested", [(0, 200), (20, 30), (70, 30), (130, 40)]),                  # six distinct breakpoints: seven intervals
    ("touching", [(0, 200), (20, 30), (50, 30), (130, 40)]),                # P1.end == P2.pos
    ("at_start", [(0, 200), (0, 30), (70, 30), (130, 40)]),                 # a partner begins at A.pos (behind A in the file)
    ("at_end", [(0, 200), (20, 30), (70, 30), (160, 40)]),                  # a partner ends at A.end
    ("before", [(0, 30), (0, 200), (70, 30), (130, 40)]),                   # a partner at A's position, earlier in the file
    ("before_two", [(0, 30), (10, 30), (10, 160), (130, 30)]),              # two partners before A in the file (they overlap at A.pos), one behind
)


def partner_lists(n_samples=1):
    """k_find_partners / plan_multi.  One contig, a name group per GROUP_SPACING positions, the samples cycling over the groups
    (all records of a group share one).  PARTNER_GROUPS: a long record A with three mutually disjoint same-name partners inside
    its span -- A is paired, alone (`past`), paired again, and counts twice where it wins -- with six distinct breakpoints
    (seven intervals), with coinciding ones, with a partner at A's first and at A's last position, with partners earlier in
    the file than A.  Then a trio of mutually overlapping records across the tile border at T, and an ordinary pair.  No
    column is covered by four records of one name and no record has more than three partners."""
    T = tile_positions(n_samples)
    mk = _Maker(760 + n_samples, n_samples)
    at = 50
    for _, parts in PARTNER_GROUPS:
        name = mk.name()
        group = mk.n % mk.S
        for k, (off, n) in enumerate(parts):
            mk.rec(0, at + off, _m(n, k & 1), name, group, mapq=20 + 10 * (k % 3))
        at += GROUP_SPACING
    at = (at // T + 2) * T
    name = mk.name()
    for k in range(3):
        mk.rec(0, at - 30 + 10 * k, "60M", name, mk.n % mk.S, mapq=20 + 10 * k)
    mk.pair(0, at + 200, "50M", at + 220, "50M")
    return [("groups", at + T)], mk.records(), read_groups_for(n_samples)


def partner_refusals():
    """Inputs K7 refuses, by name: `four_partners`: a record with four mutually disjoint same-name partners inside its span (no
    column holds more than two of them: refused because a record lists at most three partners); `four_over_one_column`: four
    same-name records over one column."""
    out = {}
    mk = _Maker(770)
    name = mk.name()
    mk.rec(0, 100, "250M", name)
    for k in range(4):
        mk.rec(0, 110 + 60 * k, "30M", name)
    out["four_partners"] = ([("c", 1024)], mk.records(), [])
    mk = _Maker(771)
    name = mk.name()
    for k in range(4):
        mk.rec(0, 100 + 10 * k, "60M", name)
    out["four_over_one_column"] = ([("c", 1024)], mk.records(), [])
    return out


# ---- one name in two samples -----------------------------------------------------------------------------------------------
def same_name_two_samples():
    """Overlapping records of one name in two samples, by name of the input; s1 and s2 are the samples, the records are in file
    order, ten positions apart, `60M` each, next to an ordinary pair:
    * `xyz`: X (s1), Y (s2), Z (s1).  In the reference's column Y sorts between X and Z, which therefore are no neighbours and
      do not pair (depth.d:343-377) where all three cover a column -- and do pair where Y does not;
    * `xyzw`: X (s1), Y (s2), Z (s1), W (s2): no pair where all four cover a column;
    * `xzy`: X (s1), Z (s1), Y (s2): X and Z are neighbours and pair; behind X's end Z stays `detected` beside Y (equal hashes,
      the loop's `past` branch is not taken) and is not counted on its own.
    A record with a partner of its own sample and an overlapping same-name record of another sample: K7 refuses all three.
    * `two`: X (s1), Y (s2) alone: nobody has a partner, nothing is refused."""
    out = {}
    for key, groups in (("xyz", (0, 1, 0)), ("xyzw", (0, 1, 0, 1)), ("xzy", (0, 0, 1)), ("two", (0, 1))):
        mk = _Maker(780 + len(out), 2)
        name = mk.name()
        for k, g in enumerate(groups):
            mk.rec(0, 100 + 10 * k, "60M", name, g)
        mk.pair(0, 400, "50M", 420, "50M")
        out[key] = ([("c", 1024)], mk.records(), read_groups_for(2))
    return out
