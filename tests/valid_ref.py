"""Is a BAM record valid?  A Python restatement of isValid / BooleanValidator (BioD bio/std/hts/bam/validation/alignment.d) and of
the parts of bam/read.d and bam/tagvalue.d it calls, written from those files.  mask(rec) returns, for the raw bytes of a record
(block_size included), the classes of error it has as a bit mask; every class is evaluated on its own.  Where the reference reads
past the record or throws the record is MALFORMED."""
import struct

CLASSES = ("name-empty", "name-chars", "position", "qualities", "cigar-hard", "cigar-soft", "cigar-length", "tag-value",
           "tag-duplicate", "malformed")
(NAME_EMPTY, NAME_CHARS, POSITION, QUALITIES, CIGAR_HARD, CIGAR_SOFT, CIGAR_LENGTH, TAG_VALUE, TAG_DUPLICATE,
 MALFORMED) = (1 << k for k in range(10))

INT_KEYS = "AM AS CM CP FI H0 H1 H2 HI IH MQ NH NM OP PQ SM TC UQ".split()
STRING_KEYS = "BC BQ CC CQ CS E2 FS LB MD OQ OC PG PU Q2 R2 RG U2".split()
QUALITY_KEYS = "CQ E2 OQ Q2 U2".split()
SIZES = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
CIGAR_TYPES = "MIDNSHP=X???????"


def tags_of(chunk):
    """([(key, type, element type or None, value)], broken): opApply of read.d, `while (offset + 1 < length)` -- one byte left over
    is not looked at.  broken: where readValueFromArray would read past the chunk or throw; the tags in front of it are returned."""
    out, off = [], 0
    while off + 1 < len(chunk):
        key = chunk[off:off + 2].decode("latin-1")
        off += 2
        if off >= len(chunk):
            return out, True                            # a key without a type
        ty = chr(chunk[off])
        off += 1
        if ty in "ZH":
            end = chunk.find(b"\0", off)
            if end < 0:
                return out, True                        # no NUL
            out.append((key, ty, None, chunk[off:end]))
            off = end + 1
        elif ty == "B":
            if off + 5 > len(chunk):
                return out, True
            sub = chr(chunk[off])
            if sub not in "cCsSiIf":
                return out, True                        # UnknownTagTypeException
            n = struct.unpack_from("<I", chunk, off + 1)[0]
            if off + 5 + n * SIZES[sub] > len(chunk):
                return out, True
            out.append((key, ty, sub, chunk[off + 5:off + 5 + n * SIZES[sub]]))
            off += 5 + n * SIZES[sub]
        else:
            if ty not in SIZES:
                return out, True                        # UnknownTagTypeException
            if off + SIZES[ty] > len(chunk):
                return out, True
            out.append((key, ty, None, chunk[off:off + SIZES[ty]]))
            off += SIZES[ty]
    return out, False


def md_valid(s):
    """alignment.d:487-520, the loop as written"""
    if not s or not chr(s[0]).isdigit():
        return False
    up = lambda c: 65 <= c <= 90
    dg = lambda c: 48 <= c <= 57
    i = 1
    while i < len(s) and dg(s[i]):
        i += 1
    while i < len(s):
        if up(s[i]):
            i += 1
        elif s[i] == ord("^"):
            i += 1
            if i == len(s) or not up(s[i]):
                return False
            while i < len(s) and up(s[i]):
                i += 1
        else:
            return False
        if i == len(s) or not dg(s[i]):
            return False
        while i < len(s) and dg(s[i]):
            i += 1
    return True


def tag_valid(key, ty, sub, v, l_seq):
    if ty == "H":
        if not v or any(chr(c) not in "0123456789abcdefABCDEF" for c in v):
            return False
    elif ty == "A":
        if not 33 <= v[0] <= 126:
            return False
    elif ty == "Z":
        if not v or any(not 32 <= c <= 126 for c in v):
            return False
    if key in INT_KEYS:
        return ty in "cCsSiI"
    if key == "FZ":
        return ty == "B" and sub == "S"
    if key in STRING_KEYS:
        if ty != "Z":
            return False
        if key in QUALITY_KEYS and v != b"*" and any(not 33 <= c <= 126 for c in v):
            return False
        if key in ("BQ", "E2") and len(v) != l_seq:
            return False
        if key == "MD" and not md_valid(v):
            return False
    return True


def name_of(rec):
    """the name `sbx-validate` reports: the l_read_name - 1 bytes, or b"" when the record does not hold them"""
    if len(rec) < 36:
        return b""
    bs, l_name = struct.unpack_from("<I", rec)[0], rec[12]
    if bs < 32 or 4 + bs > len(rec) or not l_name or 32 + l_name > bs:
        return b""
    return rec[36:36 + l_name - 1]


def mask(rec):
    if len(rec) < 36:
        return MALFORMED
    bs, _ref, pos, l_name, _mapq, _bin, n_cigar, _flag, l_seq = struct.unpack_from("<IiiBBHHHI", rec)
    if bs < 32 or bs > 0x7FFFFFF0 or 4 + bs > len(rec):
        return MALFORMED
    fixed = 32 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    if l_name == 0 or fixed > bs:
        return MALFORMED
    m = 0
    name = rec[36:36 + l_name - 1]
    if not name:
        m |= NAME_EMPTY
    if any(c < 33 or c > 126 or c == 64 for c in name):
        m |= NAME_CHARS
    if pos < -1 or pos > (1 << 29) - 2:
        m |= POSITION
    at = 36 + l_name
    ops = struct.unpack_from("<%dI" % n_cigar, rec, at)
    cigar = [(CIGAR_TYPES[o & 15], o >> 4) for o in ops]
    at += 4 * n_cigar + (l_seq + 1) // 2
    qual = rec[at:at + l_seq]
    if not all(q == 0xFF for q in qual) and not all(q <= 93 for q in qual):
        m |= QUALITIES
    if cigar:
        if len(cigar) > 2 and any(t == "H" for t, _ in cigar[1:-1]):
            m |= CIGAR_HARD
        if len(cigar) > 2:
            c = cigar
            if c[0][0] == "H":
                c = c[1:]
            if c[-1][0] == "H":
                c = c[:-1]
            if len(c) > 2 and any(t == "S" for t, _ in c[1:-1]):
                m |= CIGAR_SOFT
        if 0 < l_seq < 1 << 31 and l_seq != sum(n for t, n in cigar if t in "MIS=X") & 0xFFFFFFFF:
            m |= CIGAR_LENGTH
    tags, broken = tags_of(rec[4 + fixed:4 + bs])
    if broken:
        m |= MALFORMED
    if any(not tag_valid(k, t, s, v, l_seq) for k, t, s, v in tags):
        m |= TAG_VALUE
    keys = [k for k, _, _, _ in tags]
    if len(set(keys)) != len(keys):
        m |= TAG_DUPLICATE
    return m
