"""Pure-Python restatement of the SAM line `sambamba view` prints for a BAM record (BamRead.toSam, BioD bio/std/hts/bam/read.d:695-760;
TagValue.toSam, tagvalue.d:468-505), the test oracle of sam_core.hpp and K13.  Built from struct and "%g" % value: Python's %g is C's
for finite doubles; inf, nan and the sign of a NaN are spelled out here."""
import math
import struct

BASES = "=ACMGRSVTWYHKDBN"
CIGAR_CHARS = "MIDNSHP=X???????"
SCALARS = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}


class Malformed(Exception):
    """what the reference dies on with a range error"""


def fmt_g(bits):
    """snprintf("%g", (double)f) for the float with these 32 bits"""
    f = struct.unpack("<f", struct.pack("<I", bits))[0]
    sign = "-" if bits >> 31 else ""
    if math.isnan(f):
        return sign + "nan"
    if math.isinf(f):
        return sign + "inf"
    return "%g" % f


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >> 31 else v


def _scalar(ty, data, p):
    if ty == "f":
        return fmt_g(struct.unpack_from("<I", data, p)[0])
    return str(struct.unpack_from(SCALARS[ty], data, p)[0])


def sam_line(rec, ref_names):
    """The line, its newline included, of the record `rec` (bytes, block_size prefix first); ref_names: the names of the header."""
    n = len(rec)
    if n < 36:
        raise Malformed("short")
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq, mref, mpos, tlen = struct.unpack_from("<iiBBHHHiiii", rec, 4)
    if l_seq < 0:
        raise Malformed("l_seq")
    cig_at = 36 + l_name
    seq_at = cig_at + 4 * n_cig
    qual_at = seq_at + (l_seq + 1) // 2
    tags_at = qual_at + l_seq
    if tags_at > n:
        raise Malformed("lengths")
    for r in (ref, mref):
        if r < -1 or r >= len(ref_names):
            raise Malformed("reference id")
    f = [rec[36:36 + max(l_name - 1, 0)], b"%d" % flag, b"*" if ref == -1 else ref_names[ref].encode(), b"%d" % _wrap32(pos + 1), b"%d" % mapq]
    cig = struct.unpack_from("<%dI" % n_cig, rec, cig_at)
    f.append("".join("%d%s" % (c >> 4, CIGAR_CHARS[c & 15]) for c in cig).encode() if n_cig else b"*")
    f.append(b"*" if mref == -1 else b"=" if mref == ref else ref_names[mref].encode())
    f += [b"%d" % _wrap32(mpos + 1), b"%d" % tlen]
    if l_seq == 0:
        f += [b"*", b"*"]
    else:
        packed = rec[seq_at:qual_at]
        f.append("".join(BASES[packed[i >> 1] >> 4 if i % 2 == 0 else packed[i >> 1] & 15] for i in range(l_seq)).encode())
        q = rec[qual_at:tags_at]
        f.append(b"*" if q[0] == 0xFF else bytes((x + 33) & 0xFF for x in q))
    p = tags_at
    while p < n:
        if p + 3 > n:
            raise Malformed("tag header")
        key, ty = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if ty == "A":
            if p + 1 > n:
                raise Malformed("A")
            val = b"A:" + rec[p:p + 1]
            p += 1
        elif ty in "ZH":
            e = rec.find(b"\0", p)
            if e < 0:
                raise Malformed("no NUL")
            val = ty.encode() + b":" + rec[p:e]
            p = e + 1
        elif ty == "B":
            if p + 5 > n:
                raise Malformed("B header")
            sub, count = chr(rec[p]), struct.unpack_from("<I", rec, p + 1)[0]
            p += 5
            if sub not in SCALARS:
                raise Malformed("B type")
            size = struct.calcsize(SCALARS[sub])
            if count * size > n - p:
                raise Malformed("B count")
            val = ("B:" + sub + "," + ",".join(_scalar(sub, rec, p + k * size) for k in range(count))).encode()
            p += count * size
        elif ty in SCALARS:
            size = struct.calcsize(SCALARS[ty])
            if p + size > n:
                raise Malformed("scalar")
            val = (("f:" if ty == "f" else "i:") + _scalar(ty, rec, p)).encode()
            p += size
        else:
            raise Malformed("tag type")
        f.append(key + b":" + val)
    return b"\t".join(f) + b"\n"


def sam_text(recs, ref_names):
    return b"".join(sam_line(r, ref_names) for r in recs)
