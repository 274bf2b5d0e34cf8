"""Pure-Python restatement of a SAM alignment line turned into a BAM record, written from the grammar of parseAlignmentLine (BioD
bio/etc/ragel/sam_alignment.rl) and not from sambamba_amd/csrc/samparse_core.hpp: regular expressions for the fields, struct for the
bytes, fractions for the floats.  A line outside the grammar -- the reference would recover from it silently -- raises Malformed.

record(line, ref_names) is the record with its block_size word; float_bits(text) the binary32 a float literal rounds to (exact
rational arithmetic, ties to even: what glibc's strtof returns); header_references(text) the @SQ list of a header text.
"""
import re
import struct
from fractions import Fraction


class Malformed(Exception):
    pass


UINT = re.compile(rb"[0-9]{1,18}")
INT = re.compile(rb"[-+]?[0-9]{1,18}")
FLOAT = re.compile(rb"[-+]?(?:[0-9]*\.?[0-9]+(?:[eE][-+]?[0-9]+)?|inf)|nan|-nan")       # ("-nan": what the SAM writer prints)
QNAME = re.compile(rb"[!-?A-~]{1,254}")
REFNAME = re.compile(rb"[!-()+-<>-~][!-~]*")
CIGAR_OP = re.compile(rb"([0-9]{1,18})([MIDNSHPX=])")
SEQ = re.compile(rb"[A-Za-z=.]+")
QUAL = re.compile(rb"[!-~]+")
TAG = re.compile(rb"([A-Za-z][A-Za-z0-9]):([AifZHB]):(.*)", re.S)

BASE_CODES = {c: k for k, c in enumerate("=ACMGRSVTWYHKDBN")}
CIGAR_CODES = {c: k for k, c in enumerate("MIDNSHP=X")}
REF_CONSUMING = set("MDN=X")
ARRAY = {"c": ("<b", -128, 127), "C": ("<B", 0, 255), "s": ("<h", -32768, 32767), "S": ("<H", 0, 65535),
         "i": ("<i", -(1 << 31), (1 << 31) - 1), "I": ("<I", 0, (1 << 32) - 1)}


def _full(rx, text):
    m = rx.fullmatch(text)
    if not m:
        raise Malformed(text[:60])
    return m


def _uint(text, most):
    v = int(_full(UINT, text).group())
    if v > most:
        raise Malformed(text)
    return v


def float_bits(text):
    """the bits of the binary32 nearest to the literal (bytes), ties to even; overflow is an infinity, underflow a denormal or zero"""
    _full(FLOAT, text)
    if text == b"nan":
        return 0x7FC00000
    if text == b"-nan":
        return 0xFFC00000
    sign = 0x80000000 if text[:1] == b"-" else 0
    body = text.lstrip(b"+-")
    if body == b"inf":
        return sign | 0x7F800000
    mant, _, exp = body.lower().partition(b"e")
    whole, _, frac = mant.partition(b".")
    digits = int(whole + frac or b"0")
    if digits == 0:
        return sign
    e10 = int(exp or b"0") - len(frac)
    n_digits = len(str(digits))
    if n_digits + e10 > 40:
        return sign | 0x7F800000
    if n_digits + e10 < -50:
        return sign
    v = Fraction(digits) * Fraction(10) ** e10
    # 2^e <= v < 2^(e + 1)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    u = max(e - 23, -149)                                   # the weight of the last kept bit
    scaled = v / Fraction(2) ** u
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m & 1):
        m += 1
    if m < 1 << 23:
        return sign | m                                     # zero or a denormal
    if m == 1 << 24:
        m, u = 1 << 23, u + 1
    biased = u + 23 + 127
    if biased >= 255:
        return sign | 0x7F800000
    return sign | biased << 23 | (m - (1 << 23))


def reg2bin(beg, end):
    """bio/std/hts/bam/bai/bin.d:82-92 (Python's >> floors as D's does on an int)"""
    if end == beg:
        end = beg + 1
    end -= 1
    for shift, first in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return (first + (beg >> shift)) & 0xFFFF
    return 0


def _wrap32(v):
    return (v + (1 << 31)) % (1 << 32) - (1 << 31)


def _ref_id(text, ref_names):
    if text == b"*":
        return -1
    _full(REFNAME, text)
    try:
        return ref_names.index(text.decode("latin-1"))
    except ValueError:
        raise Malformed(b"no such reference: " + text[:60])


def _tag(text):
    key, ty, val = _full(TAG, text).groups()
    ty = ty.decode()
    if ty == "A":
        if not re.fullmatch(rb"[!-~]", val):
            raise Malformed(text)
        return key + b"A" + val
    if ty == "i":
        v = int(_full(INT, val).group())
        for letter, (fmt, lo, hi) in (("c", ARRAY["c"]), ("s", ARRAY["s"]), ("i", ARRAY["i"])) if v < 0 else (("C", ARRAY["C"]), ("S", ARRAY["S"]), ("I", ARRAY["I"])):
            if lo <= v <= hi:
                return key + letter.encode() + struct.pack(fmt, v)
        raise Malformed(text)
    if ty == "f":
        return key + b"f" + struct.pack("<I", float_bits(val))
    if ty == "Z":
        return key + b"Z" + _full(re.compile(rb"[ !-~]+"), val).group() + b"\0"
    if ty == "H":
        return key + b"H" + _full(re.compile(rb"[0-9A-Fa-f]+"), val).group() + b"\0"
    sub, rest = val[:1].decode("latin-1"), val[1:]
    if sub not in "cCsSiIf" or not sub or not rest.startswith(b","):
        raise Malformed(text)
    items = [] if rest == b"," else rest[1:].split(b",")            # ("B:c," -- no element -- is what the SAM writer prints for count 0)
    out = key + b"B" + sub.encode() + struct.pack("<I", len(items))
    for it in items:
        if sub == "f":
            out += struct.pack("<I", float_bits(it))
        else:
            v = int(_full(INT, it).group())
            fmt, lo, hi = ARRAY[sub]
            if not lo <= v <= hi:
                raise Malformed(text)
            out += struct.pack(fmt, v)
    return out


def record(line, ref_names):
    """the BAM record (block_size first) of the line (bytes, no newline); ref_names: the @SQ SN values in order"""
    f = line.split(b"\t")
    if len(f) < 11:
        raise Malformed(b"fewer than eleven fields")
    name = _full(QNAME, f[0]).group()
    flag, pos, mapq = _uint(f[1], 65535), _uint(f[3], (1 << 31) - 1), _uint(f[4], 255)
    ref = _ref_id(f[2], ref_names)
    cigar, end_pos = [], pos
    if f[5] != b"*":
        at = 0
        while at < len(f[5]):
            m = CIGAR_OP.match(f[5], at)
            if not m or int(m.group(1)) >= 1 << 28:
                raise Malformed(f[5][:60])
            n, op = int(m.group(1)), m.group(2).decode()
            cigar.append(n << 4 | CIGAR_CODES[op])
            if op in REF_CONSUMING:
                end_pos = _wrap32(end_pos + n)
            at = m.end()
        if not cigar or len(cigar) > 65535:
            raise Malformed(b"CIGAR")
    if end_pos == pos:
        end_pos += 1
    bin_ = reg2bin(_wrap32(pos - 1), _wrap32(end_pos - 1))
    mate_ref = ref if f[6] == b"=" else _ref_id(f[6], ref_names)
    mate_pos = _uint(f[7], (1 << 31) - 1)
    tlen = int(_full(INT, f[8]).group())
    if not -(1 << 31) <= tlen < 1 << 31:
        raise Malformed(f[8])
    seq = b"" if f[9] == b"*" else _full(SEQ, f[9]).group()
    packed = bytearray((len(seq) + 1) // 2)
    for k, c in enumerate(seq.decode()):
        packed[k >> 1] |= BASE_CODES.get(c.upper(), 15) << (0 if k & 1 else 4)
    q = _full(QUAL, f[10]).group()
    if q == b"*" and len(seq) != 1:
        qual = b"\xff" * len(seq)                          # (no bytes for no bases)
    elif len(q) == len(seq):
        qual = bytes(c - 33 for c in q)
    else:
        raise Malformed(b"QUAL and SEQ differ in length")
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(name) + 1, mapq, bin_, len(cigar), flag, len(seq), mate_ref, mate_pos - 1, tlen)
    body += name + b"\0" + b"".join(struct.pack("<I", c) for c in cigar) + bytes(packed) + qual
    for t in f[11:]:
        body += _tag(t)
    return struct.pack("<i", len(body)) + body


def header_references(text):
    """[(name, length)] of the @SQ lines of a header text (str), in order"""
    refs = []
    for line in text.splitlines():
        if line.startswith("@SQ\t"):
            f = dict(x.split(":", 1) for x in line.split("\t")[1:])
            refs.append((f["SN"], int(f["LN"])))
    return refs


def split_sam(data):
    """(header text, [record lines]) of SAM bytes: the header is the run of '@' lines at the top; the last line need not end in '\\n'"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    k = 0
    while k < len(lines) and lines[k].startswith(b"@"):
        k += 1
    return "".join(l.decode() + "\n" for l in lines[:k]), lines[k:]


def bam_stream(header_text, refs, records):
    """the inflated bytes of a BAM: magic, text, reference list, records"""
    out = b"BAM\1" + struct.pack("<i", len(header_text)) + header_text.encode() + struct.pack("<i", len(refs))
    for name, length in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return out + b"".join(records)
