"""Hand-made inputs of the markdup tests (tests/test_markdup_cpu.py, tests/test_gpu_markdup.py): one scenario per rule of
sambamba/markdup.d, each at positions of its own, with the duplicates written down by hand -- not derived from the restatement."""
import random

from tests import bamgen

REFS = [("c1", 100000), ("c2", 50000)]
TEXT = ("@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:c1\tLN:100000\n@SQ\tSN:c2\tLN:50000\n@RG\tID:gA\tLB:L1\tSM:s\n@RG\tID:gB\tSM:s\tLB:L1\n"
        "@RG\tID:gC\tLB:L2\tSM:s\n@PG\tID:bwa\tPN:bwa\n")
F1, R2, F2 = 0x61, 0x91, 0x81       # first mate forward (mate reverse), second mate reverse, second mate forward


def rec(name, ref, pos, cigar="10M", flag=0, qual=30, rg=None):
    l_seq = sum(n for op, n in bamgen.parse_cigar(cigar) if op in "MIS=X")
    return bamgen.make_record(ref, pos, cigar, ("ACGT" * 40)[:l_seq], qual, name=name, flag=flag,
                              tags=bamgen.tag_i("NM", 0) + (bamgen.tag_z("RG", rg) if rg is not None else b""))


def scenarios():
    """(records, labels of the duplicates, output flags to check {label: flag}, (n_end_pairs, n_single_ends, n_unmatched_pairs))."""
    r = [
        # two pairs at the same key, different scores: the weaker pair is marked
        rec("s1A", 0, 1000, flag=F1, qual=30), rec("s1A", 0, 1200, flag=R2, qual=30),
        rec("s1B", 0, 1000, flag=F1, qual=20), rec("s1B", 0, 1200, flag=R2, qual=20),
        # equal scores: the earlier pair survives
        rec("s2A", 0, 2000, flag=F1), rec("s2A", 0, 2200, flag=R2),
        rec("s2B", 0, 2000, flag=F1), rec("s2B", 0, 2200, flag=R2),
        # pairs that differ only in reversed2 (s3B) or only in coord2 (s3C): no duplicates
        rec("s3A", 0, 3000, flag=F1), rec("s3A", 0, 3200, flag=R2),
        rec("s3B", 0, 3000, flag=0x41), rec("s3B", 0, 3210, flag=F2),
        rec("s3C", 0, 3000, flag=F1), rec("s3C", 0, 3201, flag=R2),
        # a fragment at a pair's end1 key and one at its end2 key: both marked
        rec("s4P", 0, 4000, flag=F1), rec("s4P", 0, 4200, flag=R2),
        rec("s4f1", 0, 4000, qual=40), rec("s4f2", 0, 4200, flag=0x10, qual=40),
        # two fragments alone: the best survives; a lone fragment
        rec("s5a", 0, 5000, qual=20), rec("s5b", 0, 5000, qual=30),
        rec("s6", 0, 6000),
        # a fragment next to an unmatched paired read
        rec("s7f", 0, 7000, qual=40), rec("s7u", 0, 7000, flag=F1, qual=20),
        # clipped reads that share a 5' coordinate only after unclipping (forward: 8000, reverse: 8115)
        rec("s8a", 0, 8005, "5S10M", qual=30), rec("s8b", 0, 8003, "3H10M", qual=30), rec("s8c", 0, 8000, "10M", qual=40),
        rec("s8d", 0, 8100, "10M5S", flag=0x10, qual=20), rec("s8e", 0, 8105, "10M", flag=0x10, qual=35),
        # the same position in two libraries; two read groups of one library
        rec("s9a", 0, 9000, rg="gA"), rec("s9b", 0, 9000, rg="gC"),
        rec("s10a", 0, 10000, rg="gA", qual=30), rec("s10b", 0, 10000, rg="gB", qual=20),
        # an RG the header does not know groups with a read without RG (library -1)
        rec("s11a", 0, 11000, rg="zz", qual=30), rec("s11b", 0, 11000, qual=20),
        # equal names with different RG do not pair: two unmatched reads, and the fragment next to one of them is marked
        rec("s12", 0, 12000, flag=F1, rg="gA"), rec("s12", 0, 12200, flag=R2, rg="gB"), rec("s12f", 0, 12000, rg="gA", qual=40),
        # a name three times: 1st + 2nd pair, the 3rd is unmatched; the weaker pair at the same key is marked
        rec("s13", 0, 13000, flag=F1), rec("s13", 0, 13200, flag=R2), rec("s13", 0, 13000, flag=F1, qual=25),
        rec("s13B", 0, 13000, flag=F1, qual=20), rec("s13B", 0, 13200, flag=R2, qual=20),
        # mates on different contigs: s14A has its later contig first in the file (the ends are swapped), s14B not
        rec("s14A", 1, 500, flag=0x41), rec("s14A", 0, 14000, flag=F2),
        rec("s14B", 0, 14000, flag=0x41, qual=20), rec("s14B", 1, 500, flag=F2, qual=20),
        # secondary / supplementary records keep 0x400, a primary non-duplicate loses it, unmapped and unplaced records too
        rec("s15s", 0, 15000, flag=0x100 | 0x400), rec("s15x", 0, 15000, flag=0x800 | 0x400), rec("s15n", 0, 15200, flag=0x100),
        rec("s15p", 0, 15500, flag=0x400),
        rec("s16u", 0, 16000, flag=0x4 | 0x400), bamgen.make_record(-1, -1, "", "ACGT", 30, name="s16n", flag=0x4 | 0x400),
        bamgen.make_record(-1, -1, "", "ACGT", 30, name="s16m", flag=0x4),
    ]
    dups = {"s1B#0", "s1B#1", "s2B#0", "s2B#1", "s4f1#0", "s4f2#0", "s5a#0", "s7f#0", "s8b#0", "s8c#0", "s8d#0", "s10b#0", "s11b#0", "s12f#0",
            "s13B#0", "s13B#1", "s14B#0", "s14B#1"}
    flags = {"s15s#0": 0x100 | 0x400, "s15x#0": 0x800 | 0x400, "s15n#0": 0x100, "s15p#0": 0, "s16u#0": 0x4, "s16n#0": 0x4, "s16m#0": 0x4,
             "s1B#0": F1 | 0x400, "s1A#1": R2, "s7u#0": F1}
    return r, dups, flags, (12, 23, 4)


def labels(records):
    """name#occurrence of every record."""
    seen, out = {}, []
    for r in records:
        name = r[36:36 + r[12] - 1].decode()
        out.append("%s#%d" % (name, seen.get(name, 0)))
        seen[name] = seen.get(name, 0) + 1
    return out


def random_records(n, seed, shuffled):
    """About n records on 2 contigs for the differential tests: 3 read groups in 2 libraries plus no RG and an unknown RG, positions
    drawn from a few dozen values (large groups), random clips and strands, orphans, name triples, cross-contig pairs, records that
    do not take part, 0x400 pre-set on a tenth, qualities from a handful of values (ties and strict maxima)."""
    rng = random.Random(seed)
    places = [(0, p) for p in rng.sample(range(100, 90000), 30)] + [(1, p) for p in rng.sample(range(100, 40000), 12)]
    rgs = ["gA", "gB", "gC", None, "zz"]

    def one(name, flag, rg, place=None):
        ref, pos = place or rng.choice(places)
        lead = rng.choice(("", "", "", "2S", "3H", "1H2S"))
        trail = rng.choice(("", "", "", "2S", "4H", "2S1H"))
        cigar = lead + rng.choice(("10M", "10M", "4M1D6M", "5M2I3M")) + trail
        if rng.random() < 0.1:
            flag |= 0x400
        return rec(name, ref, pos, cigar, flag | (0x10 if rng.random() < 0.5 else 0), rng.choice((10, 20, 20, 30, 30, 33)), rg)

    out, k = [], 0
    while len(out) < n:
        k += 1
        name, rg, x = "q%06d" % k, rng.choice(rgs), rng.random()
        if x < 0.45:                                    # a pair, now and then on two contigs
            a = rng.choice(places)
            b = rng.choice(places) if rng.random() < 0.15 else (a[0], a[1] + rng.choice((0, 150, 300)))
            out += [one(name, 0x41, rg, a), one(name, 0x81, rg, b)]
            if rng.random() < 0.02:                     # a name triple
                out.append(one(name, 0x41, rg, a))
        elif x < 0.55:
            out.append(one(name, 0x41, rg))             # an orphan: paired, the mate is not in the file
        elif x < 0.60:
            out.append(one(name, 0x49, rg))             # the mate is unmapped: a fragment
        elif x < 0.68:
            out.append(one(name, rng.choice((0x100, 0x800, 0x4, 0x104)), rg))
        elif x < 0.72:
            out.append(bamgen.make_record(-1, -1, "", "ACGT", 30, name=name, flag=0x4 | (0x400 if rng.random() < 0.1 else 0)))
        else:
            out.append(one(name, 0, rg))
    if shuffled:
        rng.shuffle(out)
    return out
