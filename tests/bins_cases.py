"""The generated file the tests of `index -c` and `fixbins` share: about 400 sorted records over two references, with the CIGAR
shapes and the positions at which reg2bin can go wrong, and the Python statement of the bin a record should carry."""
import random
import struct

from tests import bamgen

REFS = [("chrA", (1 << 29) - 1), ("chrB", 100000)]
BLOCK = 700         # payload bytes per BGZF block of the generated files: records straddle the blocks
BATCH = "6000"      # SBX_INDEX_BATCH_BYTES that cuts the generated file into four or more read batches


def expected_bin(rec):
    """reg2bin(pos, pos + basesCovered()) of a record (block_size field included), the reference's arithmetic (bin.d:82-92,
    read.d:255-262): an unmapped read covers nothing, end == beg becomes beg + 1"""
    pos, l_name = struct.unpack_from("<iB", rec, 8)
    n_cigar, flag = struct.unpack_from("<HH", rec, 16)
    span = 0
    if not flag & 4:
        for k in range(n_cigar):
            op = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)[0]
            if op & 15 in (0, 2, 3, 7, 8):
                span += op >> 4
    beg, end = pos, pos + span
    if end == beg:
        end = beg + 1
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return (first + (beg >> shift)) & 0xFFFF
    return 0


def records(seed=7):
    """the records of the generated file, sorted: (list of record bytes, index of the first record of chrB with a position)"""
    rng = random.Random(seed)
    spec = [(100, "50M", 0), (200, "", 0), (300, "5I3S", 0), (1000, "3M%dN3M" % (1 << 27), 0), (1200, "40M", 0x4)]
    for shift in (14, 17, 20, 23, 26):
        b = 3 << shift
        spec += [(b - 2, "1M", 0), (b - 2, "2M", 0), (b - 2, "3M", 0), (b - 1, "1M", 0), (b - 1, "1M1D1M", 0), (b, "1M", 0), (b + 1, "2S4M", 0)]
    spec.append(((1 << 29) - 2, "1M", 0))
    for _ in range(300):
        spec.append((rng.randrange(0, 1 << 22), rng.choice(("36M", "10M2I20M", "5S30M", "20M%dN10M" % rng.randrange(1, 40000), "12M3D12M")), 0))
    spec.sort(key=lambda s: s[0])
    recs = [bamgen.make_record(0, pos, cigar, "ACGTAC", 30, name="a%04d" % k, flag=flag) for k, (pos, cigar, flag) in enumerate(spec)]
    recs.append(bamgen.make_record(1, -1, "", "ACGT", 30, name="nopos", flag=0x4))
    first_b = len(recs)
    recs += [bamgen.make_record(1, 10 + 97 * k, "30M", "ACGTAC", 30, name="b%04d" % k) for k in range(60)]
    recs += [bamgen.make_record(-1, -1, "", "ACGT", 30, name="u%04d" % k, flag=0x4) for k in range(25)]
    assert all(struct.unpack_from("<H", r, 14)[0] == expected_bin(r) for r in recs)
    return recs, first_b


def with_bins(recs, bins):
    """the records with the bin of record i replaced by bins[i] (a dict)"""
    out = list(recs)
    for i, b in bins.items():
        r = bytearray(out[i])
        struct.pack_into("<H", r, 14, b)
        out[i] = bytes(r)
    return out


def write(path, recs, **kw):
    kw.setdefault("block_size", BLOCK)
    return bamgen.write_bam(str(path), REFS, recs, write_index=False, **kw)


def name_of(rec):
    return rec[36:36 + rec[12] - 1].decode()
