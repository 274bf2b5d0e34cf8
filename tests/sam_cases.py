"""The records the SAM tests share (tests/test_sam_core_cpu.py on the CPU, tests/test_gpu_sam.py on the device): every field at its
edges, every tag type, and the malformed records the reference dies on.  Records are built byte by byte (raw_record), because they hold
what tests/bamgen.make_record refuses to write: l_read_name 0, positions at the ends of int32, CIGAR operation codes above 8."""
import struct

from tests import bamgen

REFS = [("c1", 100000), ("c2", 50000), ("chrWithALongerName_3", 1000)]
REF_NAMES = [n for n, _ in REFS]
TEXT = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


def raw_record(name=b"r\0", ref=-1, pos=-1, mapq=0, cigar=(), flag=4, seq_codes=(), qual=None, mref=-1, mpos=-1, tlen=0, tags=b"",
               l_seq=None):
    """name: the l_read_name bytes as they lie in the record (NUL included; b"" is l_read_name 0); cigar: raw 32-bit words;
    seq_codes: one 4-bit code per base; qual: bytes (default 30 each)."""
    n = len(seq_codes) if l_seq is None else l_seq
    packed = bytearray((len(seq_codes) + 1) // 2)
    for i, c in enumerate(seq_codes):
        packed[i >> 1] |= c << 4 if i % 2 == 0 else c
    q = bytes([30] * len(seq_codes)) if qual is None else bytes(qual)
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(name), mapq, 0, len(cigar), flag, n, mref, mpos, tlen) + bytes(name)
    body += b"".join(struct.pack("<I", c) for c in cigar) + bytes(packed) + q + tags
    return struct.pack("<i", len(body)) + body


def _codes(n):
    return [(3 * k + 1) % 16 for k in range(n)]


def edge_records():
    recs = []
    # sequence lengths: odd and even, both sides of the 8-byte store
    for n in (0, 1, 2, 7, 8, 9, 15, 16, 17, 255):
        recs.append(raw_record(name=b"seq%03d\0" % n, seq_codes=_codes(n), qual=[(7 * k) % 94 for k in range(n)]))
    # every nibble value
    recs.append(raw_record(name=b"nibbles\0", seq_codes=list(range(16)) + list(range(15, -1, -1))))
    # names of length 0 (l_read_name 0 and 1), 1, 8 and 254; no tags anywhere above
    for nm in (b"", b"\0", b"n\0", b"eightchr\0", b"N" * 254 + b"\0"):
        recs.append(raw_record(name=nm, seq_codes=_codes(3)))
    # CIGARs: none, one, the most a record can state, every operation code, the longest operation
    recs.append(raw_record(name=b"cig1\0", ref=0, pos=10, flag=0, cigar=[(5 << 4) | 0], seq_codes=_codes(5)))
    recs.append(raw_record(name=b"cigmax\0", cigar=[((k % 1000 + 1) << 4) | (k % 9) for k in range(65535)], seq_codes=_codes(4)))
    recs.append(raw_record(name=b"cigops\0", cigar=[((k + 1) << 4) | k for k in range(16)], seq_codes=_codes(2)))
    recs.append(raw_record(name=b"ciglong\0", cigar=[(((1 << 28) - 1) << 4) | 4, 1 << 4], seq_codes=_codes(1)))
    # positions, template lengths, flag, MAPQ
    for k, p in enumerate((-1, 0, INT32_MAX)):
        recs.append(raw_record(name=b"pos%d\0" % k, ref=-1, pos=p, mpos=p, tlen=(INT32_MIN, 0, INT32_MAX)[k], seq_codes=_codes(2)))
    recs.append(raw_record(name=b"flagmapq\0", flag=65535, mapq=255, seq_codes=_codes(2)))
    # qualities: 0xFF first (the whole field is '*'), 0xFF later (prints as a space), values that wrap
    recs.append(raw_record(name=b"qstar\0", seq_codes=_codes(9), qual=[0xFF] + [20] * 8))
    recs.append(raw_record(name=b"qlate\0", seq_codes=_codes(17), qual=[20] * 8 + [0xFF] + [0, 93, 222, 223, 254, 0x7F, 0x80, 0xDE]))
    # reference and mate: * *, name *, name =, name other, * name
    for k, (r, m) in enumerate(((-1, -1), (0, -1), (1, 1), (0, 2), (-1, 1))):
        recs.append(raw_record(name=b"mate%d\0" % k, ref=r, pos=100 + k, mref=m, mpos=200 + k, flag=0 if r >= 0 else 4, seq_codes=_codes(4),
                               cigar=[4 << 4] if r >= 0 else ()))
    return recs


FLOATS = [0.0, -0.0, 1e-5, 123456.5, 1234567.0, 3.4028235e38, 1e-45, float("inf"), float("nan")]
FLOAT_BITS = [0xFFC00000, 0x7F800001, 0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x49742400, 0x497423F8, 0x38D1B717, 0x7F7FFFFF]


def _f(bits):
    return struct.pack("<I", bits)


def tag_records():
    recs = []
    t = b""
    for ty, lo, hi in (("c", -128, 127), ("C", 0, 255), ("s", -32768, 32767), ("S", 0, 65535), ("i", INT32_MIN, INT32_MAX), ("I", 0, 0xFFFFFFFF)):
        t += bamgen.tag_num("a" + ty, ty, lo) + bamgen.tag_num("b" + ty, ty, hi)
    t += bamgen.tag_num("XA", "A", "!") + bamgen.tag_z("Z0", "") + bamgen.tag_z("Z1", "x" * 700)
    t += b"H0H\0" + b"H1H" + b"1AE3" * 90 + b"\0"
    recs.append(raw_record(name=b"scalars\0", seq_codes=_codes(5), tags=t))
    t = b""
    for k, sub in enumerate("cCsSiIf"):
        for count in (0, 1, 9):
            vals = FLOATS[:count] if sub == "f" else [((-1) ** j * (j + 1) * 7) % 100 if sub.isupper() else (-1) ** j * (j + 1) * 7 for j in range(count)]
            t += b"%c%dB%c" % (ord("A") + k, count, ord(sub)) + struct.pack("<I", count) + b"".join(struct.pack(bamgen_fmt(sub), v) for v in vals)
    recs.append(raw_record(name=b"arrays\0", seq_codes=_codes(8), tags=t))
    t = b"".join(b"f%df" % k + struct.pack("<f", v) for k, v in enumerate(FLOATS)) + b"".join(b"g%df" % k + _f(b) for k, b in enumerate(FLOAT_BITS))
    t += b"BfBf" + struct.pack("<I", len(FLOAT_BITS)) + b"".join(_f(b) for b in FLOAT_BITS)
    recs.append(raw_record(name=b"floats\0", seq_codes=_codes(16), tags=t))
    t = b"".join(bamgen.tag_num("%c%c" % (ord("A") + k // 10, ord("0") + k % 10), "cCsSiIf"[k % 7], k) for k in range(40))
    recs.append(raw_record(name=b"forty\0", seq_codes=_codes(7), tags=t))
    return recs


def bamgen_fmt(sub):
    return {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I", "f": "<f"}[sub]


def malformed_records():
    """{case: record}: one bad record each; every one of them passes the length checks of the read pass"""
    return {
        "unknown_tag_type": raw_record(name=b"bad\0", seq_codes=_codes(4), tags=b"XXQ" + b"\1\2\3\4"),
        "z_without_nul": raw_record(name=b"bad\0", seq_codes=_codes(4), tags=b"XXZ" + b"no end"),
        "b_count_past_end": raw_record(name=b"bad\0", seq_codes=_codes(4), tags=b"XXBi" + struct.pack("<I", 1000) + b"\0" * 12),
        "ref_id_is_n_ref": raw_record(name=b"bad\0", ref=len(REFS), pos=5, flag=0, cigar=[4 << 4], seq_codes=_codes(4)),
        "mate_ref_id_minus_2": raw_record(name=b"bad\0", mref=-2, seq_codes=_codes(4)),
    }


def good_record(k=0):
    return raw_record(name=b"good%d\0" % k, ref=0, pos=10 + k, flag=0, mapq=40, cigar=[4 << 4], seq_codes=_codes(4), tags=bamgen.tag_i("NM", k))
