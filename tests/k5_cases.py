"""Hand-placed inputs for K5 (region / window statistics, sambamba_amd/csrc/reduce.hip and engine_stats.cpp): every builder puts reads,
windows or BED lines ON something the kernels branch on instead of near it by chance.  Pure Python on tests/bamgen.py;
tests/k5_ref.py restates the three closed forms at the head of reduce.hip, tests/test_k5_cases_cpu.py checks that each case sits where
it claims to and that the restatement agrees with the oracle, tests/test_gpu_k5_edges.py compares the device with both.

`case(name)` returns a Case: refs, records (bytes, in file order, sorted by contig and position), read_groups -- what
`bamgen.write_bam(path, refs, records, read_groups=read_groups)` takes -- and what the case is run with: window sizes, BED lines as
(ref_id, start, end), coverage thresholds, the -q values, (window, overlap) pairs for the CLI alone, ranges for the API alone, and
`limit`, a one-line statement of the limit it sits on.

What the designs rely on: k_count_reads_windows takes record i of the file in lane i % 64 of wavefront i / 64 (four wavefronts to a
block), so a `runs_*` design is either a sequence every lane of which is a leader, or a short design repeated 64 times with one padding
record behind each copy: copy r begins in lane r % 64, so every phase occurs in the one file.  k_range_reduce gives a wavefront a
chunk of at most CHUNK = 16,384 positions of a range and strides it by 64 lanes; a tile is T = tile_positions(n_samples) positions.

Left out: the wrap of the 32-bit `n_bases` at 2^32, which needs a deep stack over a wide range (65,536 reads over 65,536 positions);
and `-m`, which tests/test_gpu_k7_edges.py runs."""
import functools

from tests import bamgen as bg
from tests import k3_cases as k3

CHUNK = 16384                   # range_stats: positions per RangeChunk
MAX_THRESHOLDS = 16             # kMaxThresholds
GOOD, LOW, MIN_BQ = 30, 5, 20   # base qualities on either side of -q MIN_BQ
FLAG_UNMAPPED, FLAG_DUP = 0x4, 0x400
tile_positions = k3.tile_positions
read_groups_for = k3.read_groups_for


class Case:
    def __init__(self, name, limit, refs, records, n_samples=1, windows=(), bed=(), thresholds=(), min_bqs=(0,), overlaps=(),
                 api_ranges=()):
        self.name, self.limit, self.refs, self.records, self.n_samples = name, limit, refs, records, n_samples
        self.read_groups = read_groups_for(n_samples)
        self.windows, self.bed, self.thresholds, self.min_bqs = tuple(windows), tuple(bed), tuple(thresholds), tuple(min_bqs)
        self.overlaps, self.api_ranges = tuple(overlaps), tuple(api_ranges)

    def __iter__(self):         # (refs, records, read_groups) = case
        return iter((self.refs, self.records, self.read_groups))

    def bed_text(self):
        return "".join("%s\t%d\t%d\n" % (self.refs[r][0], a, b) for r, a, b in self.bed)

    def cli_lines(self, bed_path=None):
        """The `depth` command lines of the case, without the BAM: every window size and the BED file at every -q, and for a file
        of several samples the first of each once more with --combined."""
        thr = [x for t in self.thresholds for x in ("-T", str(t))]
        out = []
        for q in self.min_bqs:
            qa = ["-q", str(q)] if q else []
            for w in self.windows:
                out.append(["window", "-w", str(w)] + qa + thr)
            if self.bed:
                out.append(["region", "-L", bed_path] + qa + thr)
        if self.n_samples > 1:
            out += [a + ["--combined"] for a in ([out[0]] if self.windows else []) + ([out[len(self.windows)]] if self.bed else [])]
        return out


class _Maker:
    """Records with a fixed base sequence; the sample cycles over the read groups unless given."""
    def __init__(self, n_samples=1):
        self.S, self.out = n_samples, []

    def add(self, ref, pos, cigar, qual=GOOD, flag=0, mapq=60, sample=None):
        cig = bg.parse_cigar(cigar)
        l_seq = sum(n for op, n in cig if op in "MIS=X")
        qual = [qual] * l_seq if isinstance(qual, int) else list(qual)
        assert len(qual) == l_seq, (cigar, len(qual))
        s = len(self.out) % self.S if sample is None else sample
        tags = bg.tag_z("RG", "g%d" % s) if self.S > 1 else b""
        self.out.append(bg.make_record(ref, pos, cig, ("ACGT" * (l_seq // 4 + 1))[:l_seq], qual, name="k%d" % len(self.out), flag=flag,
                                       mapq=mapq, tags=tags))


# ---- add_runs -------------------------------------------------------------------------------------------------------------
RUN_W = 100                     # the window size of the rotated designs
RUN_READ = "10M"
PHASES = 64


def _rotated(name, limit, design, wins_per_copy, n_samples=1, min_bqs=(0,)):
    """`design`: [(window of the copy, kind, sample)], kind in ok / low (every quality below MIN_BQ) / unm (flagged unmapped) / dup.
    64 copies, each on windows of its own and followed by ONE duplicate-flagged padding record: copy r begins in lane r % 64."""
    assert len(design) + 1 <= RUN_W - 12 and len(design) % 2 == 0       # an odd period: the copies begin in all 64 lanes
    mk = _Maker(n_samples)
    for r in range(PHASES):
        for j, (w, kind, s) in enumerate(design + [(design[-1][0], "dup", 0)]):
            mk.add(0, (r * wins_per_copy + w) * RUN_W + j, RUN_READ, qual=LOW if kind == "low" else GOOD, sample=s,
                   flag={"unm": FLAG_UNMAPPED, "dup": FLAG_DUP}.get(kind, 0))
    return Case(name, limit, [("c", PHASES * wins_per_copy * RUN_W + 50)], mk.out, n_samples, windows=(RUN_W,), min_bqs=min_bqs)


INTERRUPTED = ([(0, "low", 0)] + [(0, "ok", 0)] * 5 + [(0, "low", 0)] + [(0, "ok", 0)] * 5 + [(0, "unm", 0)] + [(0, "ok", 0)] * 5 +
               [(0, "low", 0)] * 2 + [(0, "ok", 0)] * 3 + [(0, "unm", 0), (0, "low", 0)] +
               [(1, "low", 0)] + [(1, "ok", 0)] * 4 + [(1, "low", 0)] + [(1, "ok", 0)] * 3)
ABA = [(0, "ok", s) for s in (0, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 1, 0, 0)]


def runs_all64():
    return _rotated("runs_all64", "64 records of one window per copy: a run that fills a wavefront (copy 0), ends at lane 63, "
                    "goes on from lane 0 of the next wavefront (copies 1..63), the padding record behind it not admitted",
                    [(0, "ok", 0)] * 64, 1)


def runs_interrupted():
    return _rotated("runs_interrupted", "records that are not `on` (unmapped: kind 0; with -q 20 every quality too low) at the start, "
                    "in the middle and at the end of a run, which then goes on with the SAME slot", INTERRUPTED, 2, min_bqs=(0, MIN_BQ))


def runs_aba():
    return _rotated("runs_aba", "two samples in one window: slots A A A B B A A B A B B B A A", ABA, 1, n_samples=2)


def runs_every_lane():
    mk = _Maker()
    for i in range(3 * 64 + 1):
        mk.add(0, 16 * i + 3, RUN_READ)
    return Case("runs_every_lane", "a new window at every lane: 64 leaders, 64 runs of one", [("c", 16 * 193 + 5)], mk.out, windows=(16,))


def runs_samples(n_samples):
    mk = _Maker(n_samples)
    for i in range(3 * 64 + 1):
        mk.add(0, 2 * i, RUN_READ)
    return Case("runs_samples%d" % n_samples, "%d samples alternate inside a window: every lane is a leader" % n_samples,
                [("c", 500)], mk.out, n_samples, windows=(RUN_W,))


def runs_tail():
    mk = _Maker()
    for i in range(4 * 64 + 1):
        mk.add(0, (i // 40) * RUN_W + i % 40, RUN_READ)
    return Case("runs_tail", "64 k + 1 records (257: a second block of one live lane), runs of 40", [("c", 800)], mk.out, windows=(RUN_W,))


# ---- the second window and the long-read loop -----------------------------------------------------------------------------
STR_W, STR_LEN = 16, 16 * 12 + 7           # twelve full windows and a partial one of 7 positions


def _straddle(name, limit, specials, windows=(STR_W,), copies=4, stride=48):
    """`specials`: (position, cigar, qualities) inside a copy of `stride` positions; every copy also has three plain reads in its
    first window and three in its second."""
    rows = []
    for c in range(copies):
        base = c * stride
        rows += [(base + 2 + k, "6M", GOOD) for k in range(3)] + [(base + STR_W + 2 + k, "6M", GOOD) for k in range(3)]
        rows += [(base + p, cig, q) for p, cig, q in specials]
    rows.sort(key=lambda r: r[0])
    mk = _Maker()
    for p, cig, q in rows:
        mk.add(0, p, cig, qual=q)
    return Case(name, limit, [("c", STR_LEN)], mk.out, windows=windows, min_bqs=(0, MIN_BQ), thresholds=(1, 4))


def _q(*parts):
    return [q for n, q in parts for _ in range(n)]


def straddle_left_only():
    return _straddle("straddle_left_only", "12M over the window edge at 16, its only good bases left of the edge (on0, not on1)",
                     [(10, "12M", _q((6, GOOD), (6, LOW))), (10, "12M", GOOD)])


def straddle_right_only():
    return _straddle("straddle_right_only", "12M over the window edge, its only good bases right of the edge (on1, not on0)",
                     [(10, "12M", _q((6, LOW), (6, GOOD))), (11, "12M", _q((5, LOW), (7, GOOD)))])


def straddle_neither():
    return _straddle("straddle_neither", "12M over the window edge without a good base on either side (admitted, never on)",
                     [(10, "12M", LOW), (10, "12M", GOOD), (12, "12M", LOW)])


def straddle_deletion():
    return _straddle("straddle_deletion", "a deletion over the window edge (6M4D6M from 8: D on 14..17) and one that ends at it",
                     [(8, "6M4D6M", GOOD), (8, "6M4D6M", _q((6, GOOD), (6, LOW))), (8, "6M4D6M", _q((6, LOW), (6, GOOD))),
                      (8, "4M4D6M", _q((4, LOW), (6, GOOD)))])


def straddle_skip():
    return _straddle("straddle_skip", "a reference skip over the window edge (6M4N6M from 8: N on 14..17)",
                     [(8, "6M4N6M", GOOD), (8, "6M4N6M", _q((6, GOOD), (6, LOW))), (8, "6M4N6M", _q((6, LOW), (6, GOOD)))])


def straddle_span3():
    return _straddle("straddle_span3", "50M from 5: three windows of 20 (one turn of the k0 + 2 loop), four of 16; good bases in the "
                     "third window alone, in the first alone, everywhere",
                     [(5, "50M", _q((36, LOW), (14, GOOD))), (5, "50M", _q((10, GOOD), (40, LOW))), (5, "50M", GOOD)],
                     windows=(STR_W, 20), copies=2, stride=96)


def straddle_span5():
    return _straddle("straddle_span5", "70M from 10: five windows of 16; good bases in the fifth alone, in the third alone, everywhere; "
                     "80M from 19 in the second copy runs through the last full window into the partial one (k < nw ends the loop)",
                     [(10, "70M", _q((54, LOW), (16, GOOD))), (10, "70M", _q((22, LOW), (16, GOOD), (32, LOW))), (10, "70M", GOOD),
                      (19, "80M", _q((70, LOW), (10, GOOD))), (19, "80M", GOOD)], windows=(STR_W, 20), copies=2, stride=96)


def straddle_into_partial():
    return _straddle("straddle_into_partial", "12M from 186: begins in the last full window (11), ends in the partial one (k0 + 1 == nw); "
                     "good bases in the partial window alone, in the full one alone, in both",
                     [(186, "12M", _q((6, LOW), (6, GOOD))), (186, "12M", _q((6, GOOD), (6, LOW))), (186, "12M", GOOD)], copies=1)


def straddle_in_partial():
    return _straddle("straddle_in_partial", "reads wholly in the partial window (k0 >= nw) behind reads of the last full one",
                     [(178, "6M", GOOD), (193, "5M", GOOD), (194, "4M", GOOD), (194, "2M1D2M", GOOD)], copies=1)


# ---- k_range_reduce -------------------------------------------------------------------------------------------------------
def _carpet(mk, ref, start, end, step=23):
    """Reads of 60 reference positions every `step` positions of [start, end): depth 2 to 3, every fourth with a deletion, every
    fifth with a skip, a low quality at every seventh reference position."""
    i = 0
    for p in range(start, end - 60, step):
        cig = "25M10D25M" if i % 4 == 1 else "25M10N25M" if i % 5 == 2 else "60M"
        n = 50 if cig != "60M" else 60
        mk.add(ref, p, cig, qual=[LOW if (p + k) % 7 == 0 else GOOD for k in range(n)])
        i += 1


def range_lengths(T):
    return (1, 63, 64, 65, T - 1, T, T + 1, CHUNK, CHUNK + 1)


def ranges_lengths(n_samples):
    T = tile_positions(n_samples)
    L = 2 * (CHUNK + 1) + 100
    mk = _Maker(n_samples)
    _carpet(mk, 0, 0, L)
    bed = []
    for n in (1, 63, 64, 65):
        bed += [(0, 100, 100 + n), (0, T - 1, T - 1 + n), (0, 2 * T - 32, 2 * T - 32 + n)]
    for n in (T - 1, T, T + 1):
        bed += [(0, 0, n), (0, 17, 17 + n), (0, T, T + n)]
    for n in (CHUNK, CHUNK + 1):
        bed += [(0, 0, n), (0, 5, 5 + n), (0, L - n, L)]
    return Case("ranges_lengths%d" % n_samples, "ranges of 1, 63, 64, 65 (the lane stride), T - 1, T, T + 1 (T = %d) and 16384, 16385 (the "
                "chunk: two wavefronts add into one id) positions, inside a tile and across tile edges, as BED lines and as -w" % T,
                [("r", L)], mk.out, n_samples, windows=sorted(set(range_lengths(T)) - {1}), bed=bed, thresholds=(1, 3), min_bqs=(MIN_BQ,))


def ranges_inactive_tile(n_samples):
    T = tile_positions(n_samples)
    mk = _Maker(n_samples)
    for t in (0, 2, 4):
        _carpet(mk, 0, t * T + 1, (t + 1) * T - 1, step=11)
    bed = [(0, T // 2, 2 * T + T // 2), (0, 0, 5 * T), (0, T - 1, 2 * T + 1), (0, T, 2 * T), (0, T + 7, T + 8), (0, 3 * T - 5, 4 * T + 5)]
    return Case("ranges_inactive_tile%d" % n_samples, "tiles 1 and 3 of five hold no read (slot_of == 0xFFFFFFFF) between active ones: "
                "ranges across them, inside them, and windows of T, 3T/2 and 5T/2", [("r", 5 * T)], mk.out, n_samples,
                windows=(T, 3 * T // 2, 5 * T // 2), bed=bed, thresholds=(1, 2))


def ranges_overhang():
    T = tile_positions(1)
    mk = _Maker()
    _carpet(mk, 0, T - 200, T + 100, step=9)
    mk.add(0, T + 40, "60M")                            # the last read of c0 ends with the contig
    for k in range(6):
        mk.add(1, 0, "60M")
    _carpet(mk, 1, 0, 2 * T, step=7)
    bed = [(0, T + 50, 3 * T), (0, 0, 2 * T + 5), (0, 2 * T, 2 * T + 64), (1, 0, 64), (0, T + 99, T + 101)]
    return Case("ranges_overhang", "a BED line that runs past the last tile of c0 (tile >= t_end) into what would be the first tile of "
                "c1, which is covered from position 0: none of that is c0's", [("c0", T + 100), ("c1", 2 * T)], mk.out, bed=bed,
                thresholds=(1, 6))


def ranges_zero_window_contigs():
    mk = _Maker()
    mk.add(0, 2, "5M")
    _carpet(mk, 1, 0, 5000, step=31)
    mk.add(2, 5, "20M")
    mk.add(2, 9, "20M")
    _carpet(mk, 4, 100, 4000, step=29)
    mk.add(5, 0, "6M")
    refs = [("short0", 10), ("a", 5000), ("short1", 40), ("bare", 3000), ("b", 4000), ("short2", 7)]
    return Case("ranges_zero_window_contigs", "window ids by binary search over win_base: contigs shorter than a window (with reads) in "
                "front of, between and behind contigs with windows, and a contig of 3000 without a read (no ids either)", refs, mk.out,
                windows=(50, 1000), thresholds=(1, 2))


# ---- thresholds -----------------------------------------------------------------------------------------------------------
STACK_DEPTHS = (1, 2, 3, 15, 16, 17)
STACK_AT = {d: 20 * (i + 1) for i, d in enumerate(STACK_DEPTHS)}       # depth d over [STACK_AT[d], STACK_AT[d] + 5)
THRESHOLDS_16 = (1, 2, 3, 4, 14, 15, 16, 17, 18, 2, 16, 65535, 65536, 70000, 1000000, 1)


def thresholds_stacks(n_samples):
    """Every stack belongs to ONE sample (stack i to sample i % n_samples), so the depth a threshold meets is the same in every file."""
    mk = _Maker(n_samples)
    for i, d in enumerate(STACK_DEPTHS):
        for _ in range(d):
            mk.add(0, STACK_AT[d], "5M", sample=i % n_samples)
    bed = [(0, STACK_AT[d] - 2, STACK_AT[d] + 7) for d in STACK_DEPTHS] + [(0, 0, 400), (0, 98, 103)]
    return Case("thresholds_stacks%d" % n_samples, "stacks of 1, 2, 3, 15, 16, 17 reads; 16 thresholds at once: on, one below and one "
                "above each depth, repeated ones, 65535 and above ([id][S][n_thr] with %d samples)" % n_samples, [("c", 400)],
                mk.out, n_samples, windows=(5, 10, 400), bed=bed, thresholds=THRESHOLDS_16)


def thresholds_counts():
    c = thresholds_stacks(1)
    return [Case("thresholds_none", "n_thr == 0", c.refs, c.records, windows=(10,), bed=c.bed),
            Case("thresholds_one", "n_thr == 1, the threshold on a depth", c.refs, c.records, windows=(10,), bed=c.bed, thresholds=(16,))]


def thresholds_stack300():
    mk = _Maker()
    shapes = (("8M", _q((8, GOOD))), ("3M2D3M", _q((6, GOOD))), ("3M2N3M", _q((6, GOOD))), ("8M", _q((3, GOOD), (2, LOW), (3, GOOD))),
              ("8M", _q((8, LOW))))
    for i in range(300):
        cig, q = shapes[i % 5]
        mk.add(0, 100, cig, qual=q)
    return Case("thresholds_stack300", "300 reads over 100..107, a fifth each with D, with N, with low and with only low qualities on "
                "103..104: the depth a threshold meets differs from the bases counted", [("c", 300)], mk.out, windows=(4, 100),
                bed=[(0, 100, 108), (0, 103, 105), (0, 90, 104)], thresholds=(1, 120, 121, 179, 180, 181, 240, 241, 299, 300, 301),
                min_bqs=(0, MIN_BQ))


# ---- k_count_reads_regions ------------------------------------------------------------------------------------------------
def _few_reads(mk, ref, at):
    for k in range(5):
        mk.add(ref, at + 7 * k, "30M", qual=_q((10, GOOD), (20, LOW)) if k % 2 else GOOD)


def regions_long_then_short():
    mk = _Maker()
    _few_reads(mk, 0, 5000)
    bed = [(0, 0, 15000)] + [(0, 100 + 10 * i, 105 + 10 * i) for i in range(200)] + [(0, 5010, 5012), (0, 6000, 6100)]
    return Case("regions_long_then_short", "a region of 15000 positions, then 200 short ones that end before the reads at 5000: the "
                "backward walk passes them all under pmax_end", [("c", 20000)], mk.out, bed=bed, min_bqs=(0, MIN_BQ))


def regions_duplicates():
    mk = _Maker()
    _few_reads(mk, 0, 500)
    bed = [(0, 505, 520), (0, 400, 600), (0, 505, 520), (0, 505, 520), (0, 0, 505), (0, 400, 600), (0, 519, 521)]
    return Case("regions_duplicates", "the same BED line three times and twice, unsorted and overlapping: each gets its own count",
                [("c", 2000)], mk.out, bed=bed, thresholds=(1, 3), min_bqs=(0, MIN_BQ))


def regions_touching():
    mk = _Maker()
    mk.add(0, 500, "30M")
    mk.add(0, 700, "10M5D10M")
    bed = [(0, 480, 500), (0, 480, 501), (0, 530, 540), (0, 529, 540), (0, 690, 700), (0, 725, 730), (0, 710, 715), (0, 724, 725)]
    return Case("regions_touching", "regions that end exactly at a read's start (480..500) or begin exactly at its end (530..), and the "
                "same one position further in; one that lies in a deletion", [("c", 2000)], mk.out, bed=bed, thresholds=(1,),
                api_ranges=[(0, 500, 500), (0, 510, 510), (0, 0, 0), (0, 520, 510)])


def regions_many_over_one_read():
    mk = _Maker()
    mk.add(0, 1000, "100M", qual=[GOOD if k % 3 else LOW for k in range(100)])
    mk.add(0, 1050, "20M")
    bed = [(0, 1000 + k, 1001 + k) for k in range(100)] + [(0, 990 + k, 1110 - k) for k in range(0, 50, 2)]
    return Case("regions_many_over_one_read", "125 regions over one read of 100 bases: one per base and 25 nested ones", [("c", 3000)],
                mk.out, bed=bed, min_bqs=(0, MIN_BQ))


def regions_contig_mismatch():
    mk = _Maker()
    _few_reads(mk, 0, 100)
    _few_reads(mk, 2, 100)
    _few_reads(mk, 3, 100)
    bed = [(1, 90, 200), (2, 90, 200), (1, 0, 1000), (2, 120, 125), (4, 0, 10)]
    return Case("regions_contig_mismatch", "contigs with reads and no region (0, 3), with regions and no read (1, 4), with both (2)",
                [("n%d" % k, 1000) for k in range(5)], mk.out, bed=bed, thresholds=(1,))


def regions_first_ring():
    mk = _Maker()
    _carpet(mk, 0, 0, 700, step=5)
    return Case("regions_first_ring", "window --overlap: the windows of the first ring count only reads that start at or after "
                "`min_start`, next to plain ones (CLI against the oracle only)", [("c", 700)], mk.out, overlaps=((64, 16), (100, 50), (64, 63)),
                min_bqs=(0, MIN_BQ))


# ---- zero-length shapes ---------------------------------------------------------------------------------------------------
def zero_zoo():
    refs, records, _ = k3.zero_length_zoo()
    bed = []
    for r, p in [(0, 40 + 70 * i) for i in range(12)] + [(1, p) for p in (1013, 1014, 1015, 1024)]:
        bed += [(r, p + 5, p + 15), (r, p, p + 11), (r, p + 10, p + 11), (r, p + 9, p + 60)]
    return Case("zero_zoo", "the zero-length operations of k3_cases.zero_length_zoo (a column of its own in the counters, none in "
                "countOverlappingBases) cut by window and region edges: the has_zero_ref correction of n_bases", refs, records,
                windows=(16, 50), bed=bed, thresholds=(1, 8), min_bqs=(0, MIN_BQ))


def zero_at_position_0():
    mk = _Maker()
    for cig in ("4S", "3I", "0M", "0D", "2S0N2S"):
        mk.add(0, 0, cig)
    mk.add(0, 0, "0D5M")
    mk.add(0, 0, "1M")
    mk.add(0, 3, "10M0D10M")
    return Case("zero_at_position_0", "reads at position 0 whose CIGAR consumes no reference (end - 1 would be -1: they must not be "
                "admitted) in front of reads that do", [("c", 64)], mk.out, windows=(16, 64), bed=[(0, 0, 1), (0, 0, 64), (0, 10, 14)],
                thresholds=(1, 2))


# ---- all of them ----------------------------------------------------------------------------------------------------------
RUNS_NAMES = ["runs_all64", "runs_interrupted", "runs_aba", "runs_every_lane", "runs_samples2", "runs_samples3", "runs_tail"]
STRADDLE_NAMES = ["straddle_left_only", "straddle_right_only", "straddle_neither", "straddle_deletion", "straddle_skip", "straddle_span3",
                  "straddle_span5", "straddle_into_partial", "straddle_in_partial"]
RANGES_NAMES = ["ranges_lengths1", "ranges_lengths2", "ranges_lengths3", "ranges_inactive_tile1", "ranges_inactive_tile2", "ranges_overhang",
                "ranges_zero_window_contigs"]
THRESHOLDS_NAMES = ["thresholds_stacks1", "thresholds_stacks2", "thresholds_stacks3", "thresholds_none", "thresholds_one",
                    "thresholds_stack300"]
REGIONS_NAMES = ["regions_long_then_short", "regions_duplicates", "regions_touching", "regions_many_over_one_read",
                 "regions_contig_mismatch", "regions_first_ring"]
ZERO_NAMES = ["zero_zoo", "zero_at_position_0"]
ALL_NAMES = RUNS_NAMES + STRADDLE_NAMES + RANGES_NAMES + THRESHOLDS_NAMES + REGIONS_NAMES + ZERO_NAMES


@functools.lru_cache(maxsize=None)
def case(name):
    """The Case of a name in ALL_NAMES; built once."""
    if name in ("thresholds_none", "thresholds_one"):
        return {c.name: c for c in thresholds_counts()}[name]
    for stem, builder in (("runs_samples", runs_samples), ("ranges_lengths", ranges_lengths), ("ranges_inactive_tile", ranges_inactive_tile),
                          ("thresholds_stacks", thresholds_stacks)):
        if name.startswith(stem) and name[len(stem):].isdigit():
            return builder(int(name[len(stem):]))
    c = globals()[name]()
    assert c.name == name
    return c
