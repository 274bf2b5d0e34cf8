"""Pure-Python restatement of `sambamba flagstat` (sambamba/flagstat.d), the test oracle of the device path.

count() inflates the BGZF blocks with zlib, walks the records with struct and runs the loop of computeFlagStatistics
(flagstat.d:31-58); text() prints the counters as flagstat_main does (flagstat.d:60-80, 131-143), with percent() emulated in
numpy float32: `to!float(a) / b` is a single-precision quotient, `* 100.0` a double product stored back into a float.
"""
import struct
import zlib

import numpy as np

FIELDS = ("reads", "secondary", "supplementary", "dup", "mapped", "pair_all", "first", "second", "pair_good", "pair_map",
          "single", "diff_chr", "diff_high")


def inflate(path):
    """The inflated byte stream of a BGZF file (the blocks up to the first empty one or the end of the file)."""
    data = open(path, "rb").read()
    out, off = bytearray(), 0
    while off + 18 <= len(data):
        xlen = struct.unpack_from("<H", data, off + 10)[0]
        bsize, p = None, off + 12
        while p < off + 12 + xlen:
            si1, si2, slen = data[p], data[p + 1], struct.unpack_from("<H", data, p + 2)[0]
            if si1 == 66 and si2 == 67:
                bsize = struct.unpack_from("<H", data, p + 4)[0]
            p += 4 + slen
        cdata = bsize - xlen - 19
        isize = struct.unpack_from("<I", data, off + 12 + xlen + cdata + 4)[0]
        if isize == 0:
            break
        out += zlib.decompress(data[off + 12 + xlen:off + 12 + xlen + cdata], -15)
        off += bsize + 1
    return bytes(out)


def records(stream):
    """(refID, mapq, flag, next_refID) of every record, in file order."""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    p = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, p)[0]
    p += 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, p)[0]
        p += 8 + l_name
    while p < len(stream):
        block_size, ref_id, _pos, bin_mq_nl, flag_nc, _l_seq, next_ref = struct.unpack_from("<iiiIIii", stream, p)
        yield ref_id, (bin_mq_nl >> 8) & 0xFF, flag_nc >> 16, next_ref
        p += 4 + block_size


def count_records(recs):
    c = {k: [0, 0] for k in FIELDS}
    for ref_id, mapq, flag, next_ref in recs:
        f = 1 if flag & 0x200 else 0
        c["reads"][f] += 1
        if not flag & 0x4:
            c["mapped"][f] += 1
        if flag & 0x400:
            c["dup"][f] += 1
        if flag & 0x100:
            c["secondary"][f] += 1
        elif flag & 0x800:
            c["supplementary"][f] += 1
        elif flag & 0x1:
            c["pair_all"][f] += 1
            if flag & 0x2 and not flag & 0x4:
                c["pair_good"][f] += 1
            if flag & 0x40:
                c["first"][f] += 1
            if flag & 0x80:
                c["second"][f] += 1
            if flag & 0x8 and not flag & 0x4:
                c["single"][f] += 1
            if not flag & 0x4 and not flag & 0x8:
                c["pair_map"][f] += 1
                if ref_id != next_ref:
                    c["diff_chr"][f] += 1
                    if mapq >= 5:
                        c["diff_high"][f] += 1
    return {k: tuple(v) for k, v in c.items()}


def count(path):
    """{counter: (QC-passed, QC-failed)} of the BAM at `path`."""
    return count_records(records(inflate(path)))


def percent(a, b):
    return np.float32(float(np.float32(a) / np.float32(b)) * 100.0)


def percent_str(a, b):
    if b == 0:
        return "N/A"
    return "%.2f%%" % float(percent(a, b))


def text(c, tabular=False):
    lines = []

    def param(what, v):
        lines.append("%s,%d,%d" % (what, v[0], v[1]) if tabular else "%d + %d %s" % (v[0], v[1], what))

    def with_pct(what, v, total):
        p0, p1 = percent_str(v[0], total[0]), percent_str(v[1], total[1])
        lines.append("%s,%d:%s,%d:%s" % (what, v[0], p0, v[1], p1) if tabular else "%d + %d %s (%s:%s)" % (v[0], v[1], what, p0, p1))

    param("in total (QC-passed reads + QC-failed reads)", c["reads"])
    param("secondary", c["secondary"])
    param("supplementary", c["supplementary"])
    param("duplicates", c["dup"])
    with_pct("mapped", c["mapped"], c["reads"])
    param("paired in sequencing", c["pair_all"])
    param("read1", c["first"])
    param("read2", c["second"])
    with_pct("properly paired", c["pair_good"], c["pair_all"])
    param("with itself and mate mapped", c["pair_map"])
    with_pct("singletons", c["single"], c["pair_all"])
    param("with mate mapped to a different chr", c["diff_chr"])
    param("with mate mapped to a different chr (mapQ>=5)", c["diff_high"])
    return "".join(line + "\n" for line in lines)
