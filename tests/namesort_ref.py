"""Pure-Python restatement of `sambamba sort -n / -N / -M` (sambamba/sort.d:221-298), the test oracle of sbx_sort_bam_by_name.

Orders (BioD bio/std/hts/bam/read.d:1493-1621), applied by Python's stable sorted() through functools.cmp_to_key:
  -n  compareReadNames: names as byte strings, a proper prefix first.
  -N  mixedStrCompare: see mixed_str_compare below, a line-by-line restatement.
  -M  among equal names: ascending HI tag (absent: 0), then ascending flag.
Whatever compares equal keeps file order.  The header is the one of tests/sort_ref.py with SO:queryname in the place of SO:coordinate;
the binary reference list and the record bytes are the input's.
"""
import functools
import struct

from tests import sort_ref
from tests.flagstat_ref import inflate

LEX, NATURAL = 1, 2


def _is_digit(c):
    return 0x30 <= c <= 0x39


def _signed(c):
    return c - 256 if c >= 128 else c


def mixed_str_compare(a, b):
    """mixedStrCompare on two bytes objects (read.d:1512-1548)."""
    i, j = 0, 0
    while i < len(a) and j < len(b):
        if _is_digit(a[i]) and _is_digit(b[j]):
            za = zb = 0
            while i < len(a) and a[i] == 0x30:
                za += 1
                i += 1
            while j < len(b) and b[j] == 0x30:
                zb += 1
                j += 1
            while i < len(a) and j < len(b) and _is_digit(a[i]) and a[i] == b[j]:
                i += 1
                j += 1
            da = i < len(a) and _is_digit(a[i])
            db = j < len(b) and _is_digit(b[j])
            if da and db:
                k, maxk = 0, min(len(a) - i, len(b) - j)
                while k < maxk and _is_digit(a[i + k]) and _is_digit(b[j + k]):
                    k += 1
                if i + k < len(a) and _is_digit(a[i + k]):
                    return 1
                if j + k < len(b) and _is_digit(b[j + k]):
                    return -1
                return _signed(a[i]) - _signed(b[j])
            if da:
                return 1
            if db:
                return -1
            if za != zb:
                return za - zb
        else:
            if a[i] != b[j]:
                return _signed(a[i]) - _signed(b[j])
            i += 1
            j += 1
    return 1 if i < len(a) else -1 if j < len(b) else 0


def name_of(rec):
    return rec[36:36 + rec[12] - 1]


def flag_of(rec):
    return struct.unpack_from("<I", rec, 16)[0] >> 16


def aux_of(rec):
    l_name = rec[12]
    n_cigar = struct.unpack_from("<H", rec, 16)[0]
    l_seq = struct.unpack_from("<i", rec, 20)[0]
    return rec[36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq:]


INT_TYPES = {b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I"}
SIZES = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}


def hi_of(rec):
    """getHI: the value of the first HI tag, 0 when there is none; ValueError when to!int would throw (or the tags are broken)."""
    aux, t = aux_of(rec), 0
    while t < len(aux):
        if t + 3 > len(aux):
            raise ValueError("tag runs past the record")
        key, ty = aux[t:t + 2], aux[t + 2:t + 3]
        t += 3
        if key == b"HI":
            if ty not in INT_TYPES or t + SIZES[ty] > len(aux):
                raise ValueError("HI is not an integer")
            v = struct.unpack_from(INT_TYPES[ty], aux, t)[0]
            if v > 0x7FFFFFFF:
                raise ValueError("HI does not fit int")
            return v
        if ty in SIZES:
            t += SIZES[ty]
        elif ty in (b"Z", b"H"):
            t = aux.index(b"\0", t) + 1                  # (ValueError when it is not terminated)
        elif ty == b"B" and t + 5 <= len(aux) and aux[t:t + 1] in SIZES and aux[t:t + 1] != b"A":
            t += 5 + struct.unpack_from("<I", aux, t + 1)[0] * SIZES[aux[t:t + 1]]
        else:
            raise ValueError("unknown tag type")
        if t > len(aux):
            raise ValueError("tag runs past the record")
    return 0


def comparator(order, match_mates):
    def cmp(x, y):
        a, b = name_of(x), name_of(y)
        c = mixed_str_compare(a, b) if order == NATURAL else (a > b) - (a < b)
        if c or not match_mates:
            return c
        hx, hy = hi_of(x), hi_of(y)
        if hx != hy:
            return -1 if hx < hy else 1
        return flag_of(x) - flag_of(y)
    return cmp


def header_text(text):
    out = sort_ref.header_text(text)
    first, rest = out.split("\n", 1)
    assert first.endswith("\tSO:coordinate")
    return first[:-len("coordinate")] + "queryname\n" + rest


def expected_stream(stream, order, match_mates=False, keep=None):
    """The inflated stream `sambamba sort -n|-N [-M]` writes for the inflated input `stream`."""
    text, refs, _, recs = sort_ref.split_stream(stream)
    if keep is not None:
        recs = [r for r in recs if keep(r)]
    recs = sorted(recs, key=functools.cmp_to_key(comparator(order, match_mates)))
    new_text = header_text(text.decode()).encode()
    return b"BAM\1" + struct.pack("<i", len(new_text)) + new_text + refs + b"".join(recs)


def expected(path, order, match_mates=False, keep=None):
    return expected_stream(inflate(path), order, match_mates, keep)
