"""Hand-placed inputs for K9 (`sambamba sort`, sambamba_amd/csrc/sort.hip): every builder puts records ON one of the limits the
kernels hard-code instead of near it by chance.  Pure Python on tests/bamgen.py; tests/test_k9_cases_cpu.py checks that each case
still sits where its docstring says (and that a model of K9b with one defect switched on gets a named case wrong),
tests/test_gpu_k9_edges.py compares the device with tests/sort_ref.py on them.

The limits: K9b's tile of TILE = 4096 elements (kRadixTile), taken in rounds of ROUND = 256 lanes, four waves of WAVE = 64; K9a's
groups of GROUP = 256 records (kSortKeysThreads); K9c's sixteen lanes per record (kCopyGroup) that move 256 bytes per trip of the
chunk loop.  The index of a record in the file is the index of its lane: record i is lane i % 256 of round (i % 4096) / 256 of tile
i / 4096 in the FIRST pass of the sort (later passes see the order the pass before left), and lane i % 256 of group i / 256 in K9a.

`case(name)` returns a Case: refs, records (bytes, in file order), the -F filter and its Python restatement, and `expect` -- the
stats the device must report, computed here from the keys of the kept records with a restatement of sort_core.hpp's `sort_key` and
`plan_passes`.  Record names carry the file index (`<letter><index>`), so a stability error shows in the bytes."""
import functools
import random
import struct

from tests import bamgen as bg

TILE, ROUND, WAVE, GROUP = 4096, 256, 64, 256
COPY_LANES = 16
MAX_LN = 2 ** 31 - 1                # the longest contig a BAM header can state
BAI_END = 1 << 29                   # the coordinate limit of the BAI's bins
BASES = "ACGTACGTAC"


# ---- sort_core.hpp, restated ----------------------------------------------------------------------------------------------
def sort_key(ref, pos, flag, n_ref):
    if ref < 0:
        return (n_ref & 0xFFFFFFFF) << 33
    return (ref & 0xFFFFFFFF) << 33 | ((pos + 1) & 0xFFFFFFFF) << 1 | ((flag >> 4) & 1)


def plan_passes(varying):
    """(shifts, key_bits): digits of 8 bits from the lowest varying bit on, a digit without a varying bit skipped."""
    if not varying:
        return [], 0
    lo = (varying & -varying).bit_length() - 1
    hi = varying.bit_length()
    return [s for s in range(lo, hi, 8) if (varying >> s) & 0xFF], hi - lo


def key_of_record(rec, n_ref):
    ref, pos = struct.unpack_from("<ii", rec, 4)
    return sort_key(ref, pos, struct.unpack_from("<I", rec, 16)[0] >> 16, n_ref)


def fields_of_record(rec):
    """(ref_id, position, flag)"""
    ref, pos = struct.unpack_from("<ii", rec, 4)
    return ref, pos, struct.unpack_from("<I", rec, 16)[0] >> 16


class Case:
    def __init__(self, name, refs, records, flt=None, keep=None):
        self.name, self.refs, self.records, self.flt, self.keep = name, refs, records, flt, keep
        kept = [r for r in records if keep is None or keep(r)]
        self.keys = [key_of_record(r, len(refs)) for r in kept]         # of the kept records, in file order
        k_or, k_and = 0, (1 << 64) - 1
        for k in self.keys:
            k_or |= k
            k_and &= k
        self.varying = (k_or ^ k_and) if self.keys else 0
        self.shifts, bits = plan_passes(self.varying)
        self.expect = {"n_records_in": len(records), "n_records_out": len(kept), "n_sort_passes": len(self.shifts), "key_bits": bits}

    def write(self, path):
        return bg.write_bam(path, self.refs, self.records, write_index=False)


def rec(i, ref, pos, strand=0, letter="r", flag=0, cigar=None, n_bases=None):
    """Record i of its file: 4 to 10 bases, no tags, the name `<letter><i>`.  A record without a contig or a position is flagged
    unmapped and has no CIGAR."""
    seq = BASES[:4 + i % 7 if n_bases is None else n_bases]
    if ref < 0 or pos < 0:
        flag |= 0x4
        cigar = ""
    elif cigar is None:
        cigar = "%dM" % len(seq)
    far = pos >= BAI_END            # beyond the binning scheme (bamgen's bin would not fit 16 bits): made at 0, the position patched
    r = bg.make_record(ref, 0 if far else pos, cigar, seq, 30, name="%s%05d" % (letter, i), flag=flag | (0x10 if strand else 0),
                       mapq=0 if flag & 0x4 else 30)
    return r[:8] + struct.pack("<i", pos) + r[12:] if far else r


# ---- 1. record counts ------------------------------------------------------------------------------------------------------
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 12289)


def count_case(n):
    """n records on one contig, the positions strictly descending in file order (n - 1 .. 0): every record moves, the output is the
    file reversed.  The radix passes see a partial wave (63, 65), a partial round (255, 257), a partial tile (4095, 4097, 8191,
    8193, 12289: the break at `t0 + r * 256 >= n` after 1 .. 16 rounds); the gather sees n % 16 in {0, 1, 15}."""
    return Case("count%d" % n, [("c1", 100000)], [rec(i, 0, n - 1 - i) for i in range(n)])


def two_equal():
    """Two records with the same key: nothing varies, 0 passes, file order."""
    return Case("two_equal", [("c1", 100000)], [rec(i, 0, 77) for i in range(2)])


# ---- 2. pass plans ---------------------------------------------------------------------------------------------------------
def _shuffled(seed, items):
    items = list(items)
    random.Random(seed).shuffle(items)
    return items


def _plan_case(name, refs, triples, seed):
    """(ref, pos, strand) triples, shuffled, every one twice at least so that ties are in the file."""
    triples = _shuffled(seed, triples)
    return Case(name, refs, [rec(i, r, p, s, cigar=("1M3S" if p > MAX_LN - 16 else None), n_bases=(4 if p > MAX_LN - 16 else None))
                             for i, (r, p, s) in enumerate(triples)])


def _spread(width, n, seed):
    """n values of `pos + 1` in [1, 2^width - 2] with 1 and 2^width - 2 among them (together they vary in all `width` bits), with
    repeats."""
    rng = random.Random(seed)
    top = (1 << width) - 2
    vals = [1, top] + [rng.randrange(1, top + 1) for _ in range(n // 2 - 2)]
    return vals + [rng.choice(vals) for _ in range(n - len(vals))]


def plan_cases():
    """name -> Case; the plan each must give is in PLAN_SHIFTS (name -> (shifts, key_bits)).
    * shift0: positions 0..126, both strands: keys 2..255, one pass at shift 0;
    * unaligned: forward strand, pos + 1 = 16 m, m in 1..255: bits 5..12 vary, one pass at shift 5;
    * overhang: m in 1..511: bits 5..13, passes at 5 and 13 -- the top digit holds one varying bit and reaches up to bit 20;
    * width8 / 9 / 16 / 17 / 25: forward strand, pos + 1 in [1, 2^w - 2]: a stretch of exactly w bits from bit 1 on, 1 / 2 / 2 / 3 / 4
      passes (4,097 records for 17: the third pass runs over two tiles and one element);
    * skipped: positions 0..126 on the contigs 0..3: bits 0..7 and 33..34, passes at 0 and 32 -- the digits at 8, 16, 24 are skipped;
    * strand: 8,193 records at one position, both strands: one pass, two digits, over two tiles and one element of a third;
    * refbit: two contigs, one position, one strand: one pass at shift 33;
    * unmapped: records without a contig (any position, any strand: they all compare equal) and ONE mapped record, last but one
      in the file;
    * two_long: two contigs of 2^31 - 1, positions up to 2^31 - 2, both strands: bits 0..31 and 33, five passes;
    * widest: 300 contigs of 2^31 - 1, positions up to 2^31 - 2, both strands, and records without a contig (key 300 << 33): bits
      0..41 (bit 32 is constant: pos + 1 < 2^31 -- the digit at 32 still varies in bits 33..39), six passes."""
    out = {}
    c1 = [("c1", MAX_LN)]
    out["shift0"] = _plan_case("shift0", c1, [(0, p, s) for p in range(127) for s in (0, 1)] * 2, 1)
    out["unaligned"] = _plan_case("unaligned", c1, [(0, 16 * m - 1, 0) for m in range(1, 256)] * 2, 2)
    out["overhang"] = _plan_case("overhang", c1, [(0, 16 * m - 1, 0) for m in range(1, 512)] * 2, 3)
    for w, n in ((8, 600), (9, 600), (16, 900), (17, 4097), (25, 900)):
        out["width%d" % w] = _plan_case("width%d" % w, c1, [(0, v - 1, 0) for v in _spread(w, n, 10 + w)], 20 + w)
    four = [("k%d" % k, 1000) for k in range(4)]
    out["skipped"] = _plan_case("skipped", four, [(r, p, s) for r in range(4) for p in range(0, 127, 3) for s in (0, 1)] * 2, 4)
    rng = random.Random(5)
    out["strand"] = Case("strand", c1, [rec(i, 0, 500, rng.randrange(2)) for i in range(2 * TILE + 1)])
    out["refbit"] = Case("refbit", four[:2], [rec(i, rng.randrange(2), 40) for i in range(700)])
    recs = [rec(i, -1, rng.choice((-1, 0, 7, 100000)), rng.randrange(2), letter="u") for i in range(500)]
    recs[-2] = rec(len(recs) - 2, 1, 123, 1, letter="m")
    out["unmapped"] = Case("unmapped", four, recs)
    two = [("long0", MAX_LN), ("long1", MAX_LN)]
    top = MAX_LN - 1
    tri = [(0, 0, 0), (1, top, 1), (0, top, 0), (1, 0, 1)] + [(rng.randrange(2), rng.randrange(top + 1), rng.randrange(2)) for _ in range(400)]
    out["two_long"] = _plan_case("two_long", two, tri + tri[:300], 6)
    many = [("w%d" % k, MAX_LN) for k in range(300)]
    tri = [(0, 0, 0), (299, top, 1), (255, top, 0), (44, 0, 1), (-1, -1, 0), (-1, 5, 1)]
    tri += [(rng.randrange(300), rng.randrange(top + 1), rng.randrange(2)) for _ in range(500)] + [(-1, rng.randrange(9), 1) for _ in range(40)]
    out["widest"] = _plan_case("widest", many, tri + tri[:350], 7)
    return out


PLAN_SHIFTS = {
    "shift0": ([0], 8), "unaligned": ([5], 8), "overhang": ([5, 13], 9),
    "width8": ([1], 8), "width9": ([1, 9], 9), "width16": ([1, 9], 16), "width17": ([1, 9, 17], 17), "width25": ([1, 9, 17, 25], 25),
    "skipped": ([0, 32], 35), "strand": ([0], 1), "refbit": ([33], 1), "unmapped": (None, None),       # (unmapped: from the keys)
    "two_long": ([0, 8, 16, 24, 32], 34), "widest": ([0, 8, 16, 24, 32, 40], 42),
}


# ---- 3. digit layouts of a single pass -------------------------------------------------------------------------------------
def _fill(i):
    """a digit in 2..251 for the lanes a layout says nothing about: the special digits 0, 1, 252..255 are never among them"""
    return 2 + (i * 37 + (i >> 8) * 11) % 250


def _digits_case(name, digits):
    """One contig; record i holds the key `digits[i]`: position (d >> 1) - 1 (-1: a record of the contig without a position) and
    strand d & 1.  The plan is one pass at shift 0 (the CPU test checks it), so lane i of the pass extracts digits[i]."""
    return Case(name, [("c1", 1000)], [rec(i, 0, (d >> 1) - 1, d & 1) for i, d in enumerate(digits)])


def layout_digits():
    """name -> the digit of every lane, in file order.
    * uniform_rounds (4096 + 512): every round of 256 lanes holds ONE digit, the next round another, the same again three rounds
      later (all four waves count 64, `off` moves on by 256);
    * everywhere (3 tiles): digit 77 in every round of every tile, in a third of the lanes, the lanes moving by one per round;
    * descending (3 rounds): lane l holds 255 - l, the next round the same again, the third l;
    * lanes_0_63: digit 253 only in lanes 0 and 63 of wave 1 of the middle round;
    * wave_edge: digit 252 only in lane 63 of wave 0 and lane 0 of wave 1 of the middle round;
    * wave3_alone (3 rounds): digit 254 all over waves 0..2 of the first round, in wave 3 alone in the second (stale counts of the
      waves in front would be added), in wave 0 alone in the third;
    * extremes: 255 and 0 alternate in wave 2 of the middle round, 0 and 255 occur nowhere else in that round;
    * dead_lanes (256 + 10): the last round has ten live lanes, all digit 0, which also occurs in the full round before;
    * last_lane (4096 + 257): digit 255 once, in the last live lane of the file."""
    out = {}
    out["uniform_rounds"] = [(11, 200, 94)[g % 3] for g in range(TILE // ROUND + 2) for _ in range(ROUND)]
    out["everywhere"] = [77 if (i % ROUND + i // ROUND) % 3 == 0 else _fill(i) for i in range(3 * TILE)]
    out["descending"] = [255 - l for l in range(ROUND)] * 2 + list(range(ROUND))
    d = [_fill(i) for i in range(3 * ROUND)]
    d[ROUND + WAVE] = d[ROUND + 2 * WAVE - 1] = 253
    out["lanes_0_63"] = d
    d = [_fill(i) for i in range(3 * ROUND)]
    d[ROUND + WAVE - 1] = d[ROUND + WAVE] = 252
    out["wave_edge"] = d
    d = [_fill(i) for i in range(3 * ROUND)]
    for l in range(ROUND):
        if l < 3 * WAVE and l % 2 == 0:
            d[l] = 254
        if l >= 3 * WAVE and l % 3 != 1:
            d[ROUND + l] = 254
        if l < WAVE and l % 5 == 0:
            d[2 * ROUND + l] = 254
    out["wave3_alone"] = d
    d = [_fill(i) for i in range(3 * ROUND)]
    for l in range(2 * WAVE, 3 * WAVE):
        d[ROUND + l] = 255 if l % 2 == 0 else 0
    d[5] = 0
    d[2 * ROUND + 9] = 255
    out["extremes"] = d
    d = [_fill(i) for i in range(ROUND)]
    d[3] = d[100] = d[255] = 0
    out["dead_lanes"] = d + [0] * 10
    out["last_lane"] = [_fill(i) for i in range(TILE + ROUND)] + [255]
    return out


# ---- 4. K9a under -F -------------------------------------------------------------------------------------------------------
FILTER = "not duplicate"
FILTER_N = 2 * GROUP + GROUP // 2


def keep_not_duplicate(record):
    return not (struct.unpack_from("<I", record, 16)[0] >> 16) & 0x400


def filter_keeps():
    """name -> keep / reject of every record by lane, over 2.5 groups of 256 records (640) unless said otherwise."""
    n = FILTER_N
    mixed = lambda i: (i * 7 + i // 5) % 3 != 0
    out = {
        "group_rejected": [not GROUP <= i < 2 * GROUP and mixed(i) for i in range(n)],
        "lane0_only": [i % GROUP == 0 if GROUP <= i < 2 * GROUP else mixed(i) for i in range(n)],
        "lane255_only": [i % GROUP == GROUP - 1 if GROUP <= i < 2 * GROUP else mixed(i) for i in range(n)],
        "wave2_rejected": [not (GROUP <= i < 2 * GROUP and (i % GROUP) // WAVE == 2) for i in range(n)],
        "alternating": [i % 2 == 1 for i in range(n)],
        "all_kept": [True] * n,
        "first_group_empty": [i >= GROUP and mixed(i) for i in range(GROUP + GROUP // 2)],     # nothing in front of a partial last group
        "one_kept": [i == GROUP + 44 for i in range(n)],
        "none_kept": [False] * n,
    }
    return out


def filter_case(name, keeps):
    """Kept records: contig 0, positions 0..60, both strands (keys in bits 0..6: one pass).  REJECTED records are flagged duplicate
    and lie on contig 1 at positions around 2^20: if one of them reached the OR / AND words, bit 33 and bits up to 21 would vary and
    `key_bits` / `n_sort_passes` would not be those of the kept keys."""
    recs = []
    for i, k in enumerate(keeps):
        if k:
            recs.append(rec(i, 0, (i * 37) % 61, (i >> 1) & 1, letter="k"))
        else:
            recs.append(rec(i, 1, (1 << 20) + (i * 13) % 977, i & 1, letter="x", flag=0x400))
    return Case("filter_" + name, [("c1", 100000), ("c2", 1 << 22)], recs, flt=FILTER, keep=keep_not_duplicate)


# ---- 5. K9c alignments -----------------------------------------------------------------------------------------------------
GATHER_N = 3000


def gather_case():
    """3,000 records at distinct positions (no ties: names of under six bytes cannot carry the index) in shuffled order, their
    lengths varying through the name (1 to 254 bytes with the NUL: `<letter><index>` padded with `x`, cut to the length) and
    the sequence: 37 bytes (no name, no CIGAR, no sequence: the shortest record bamgen makes) up to 13,500; most between 37 and
    330, so that chunk counts 0, 1, 15, 16 and 17 are common; a few above 272 + 16 (a second trip of the chunk loop for some lane),
    above 4,352 (a seventeenth) and above 32 chunks."""
    rng = random.Random(99)
    n = GATHER_N
    positions = list(range(n))
    rng.shuffle(positions)
    recs = []
    for i in range(n):
        k = rng.random()
        if i == 0:
            l_name, l_seq = 1, 0
        elif k < 0.70:
            l_name, l_seq = rng.randrange(1, 255), rng.choice((0, 0, 1, 2, 3, 4, 7, 10))
        elif k < 0.97:
            l_name, l_seq = rng.randrange(1, 60), rng.randrange(100, 200)
        elif k < 0.99:
            l_name, l_seq = rng.randrange(1, 255), rng.randrange(400, 700)
        else:
            l_name, l_seq = rng.randrange(1, 255), rng.randrange(2900, 9000)
        name = ("g%05d" % i + "x" * 254)[:l_name - 1]
        seq = "".join(rng.choice("ACGT") for _ in range(l_seq))
        flag = (0x10 if i & 1 else 0) | (0 if l_seq else 0x4)
        recs.append(bg.make_record(0, positions[i], "%dM" % l_seq if l_seq else "", seq, 20 + i % 20, name=name, flag=flag,
                                   mapq=30 if l_seq else 0))
    return Case("gather", [("c1", 100000)], recs)


def copy_span16_parts(dst, nbytes):
    """(head, chunks, tail) of copy_span16 for a destination address `dst` (only dst & 15 matters) and nbytes."""
    head = min((16 - (dst & 15)) & 15, nbytes)
    return head, (nbytes - head) >> 4, (nbytes - head) & 15


# ---- 6. a name order: K14 over K9b -----------------------------------------------------------------------------------------
def name_words_lex(name):
    """The key words of a name in the order of `sort -n`: its bytes, eight per word, the first byte the most significant, padded
    with zeros (namesort_core.hpp; tests/test_k9_cases_cpu.py compares with tests/native/namesort_host.cpp)."""
    b = name.encode()
    return [int.from_bytes(b[k:k + 8].ljust(8, b"\0"), "big") for k in range(0, len(b), 8)]


def name_case():
    """900 records with names of sixteen bytes, two key words: `<permuted index, 8 digits>` + `0000000<one of @..O>`.  The order
    sorts word 1 first: its last byte alone varies, in bits 0..3 -- ONE pass, so the permutation is left in the second value
    buffer; then word 0, whose four last digits vary: bits 0..27 (a digit varies in its four low bits), four passes that start
    from that buffer.  `expect` holds the sums."""
    n = 900
    recs, names = [], []
    for i in range(n):
        nm = "%08d" % ((i * 7919) % 9973) + "0000000" + "@ABCDEFGHIJKLMNO"[(i * 5 + i // 16) % 16]
        names.append(nm)
        seq = BASES[:4 + i % 7]
        recs.append(bg.make_record(i % 2, 5000 - i, "%dM" % len(seq), seq, 30, name=nm, flag=0x10 if i % 3 == 0 else 0))
    c = Case("names", [("c1", 100000), ("c2", 100000)], recs)
    words = [name_words_lex(nm) for nm in names]
    per_word = []
    for w in (1, 0):                                    # the order of the sort: the last word first
        k_or, k_and = 0, (1 << 64) - 1
        for ws in words:
            k_or |= ws[w]
            k_and &= ws[w]
        per_word.append(plan_passes(k_or ^ k_and))
    c.names, c.words, c.per_word = names, words, per_word
    c.expect = dict(c.expect, n_sort_passes=sum(len(s) for s, _ in per_word), key_bits=sum(b for _, b in per_word))
    return c


# ---- all of them -----------------------------------------------------------------------------------------------------------
COUNT_NAMES = ["count%d" % n for n in COUNTS] + ["two_equal"]
PLAN_NAMES = list(PLAN_SHIFTS)
LAYOUT_NAMES = ["uniform_rounds", "everywhere", "descending", "lanes_0_63", "wave_edge", "wave3_alone", "extremes", "dead_lanes", "last_lane"]
FILTER_NAMES = ["filter_" + k for k in ("group_rejected", "lane0_only", "lane255_only", "wave2_rejected", "alternating", "all_kept",
                                        "first_group_empty", "one_kept", "none_kept")]
COORDINATE_NAMES = COUNT_NAMES + PLAN_NAMES + LAYOUT_NAMES + FILTER_NAMES + ["gather"]


@functools.lru_cache(maxsize=None)
def _plans():
    return plan_cases()


@functools.lru_cache(maxsize=None)
def case(name):
    """The Case of a name in COORDINATE_NAMES, or "names"; built once."""
    if name == "two_equal":
        return two_equal()
    if name.startswith("count"):
        return count_case(int(name[5:]))
    if name in PLAN_SHIFTS:
        return _plans()[name]
    if name in LAYOUT_NAMES:
        return _digits_case(name, layout_digits()[name])
    if name.startswith("filter_"):
        return filter_case(name[7:], filter_keeps()[name[7:]])
    if name == "gather":
        return gather_case()
    if name == "names":
        return name_case()
    raise KeyError(name)
