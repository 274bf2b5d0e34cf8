"""Hand-made BAM records for the validity rules (sambamba_amd/csrc/valid_core.hpp, tests/valid_ref.py), each with the mask it must
get WRITTEN DOWN, not computed: cases() is a list of (label, record bytes, mask).  At every boundary a rule has there is a record on
either side."""
import struct

(NAME_EMPTY, NAME_CHARS, POSITION, QUALITIES, CIGAR_HARD, CIGAR_SOFT, CIGAR_LENGTH, TAG_VALUE, TAG_DUPLICATE,
 MALFORMED) = (1 << k for k in range(10))
OK = 0
OPS = "MIDNSHP=X"


def cig(text):
    """'3S5M' -> [(4, 3), (0, 5)]; a digit in place of the letter is a raw operation code: '5M2:9' = 5M then length 2, code 9"""
    out, num, i = [], "", 0
    while i < len(text):
        ch = text[i]
        if ch.isdigit():
            num += ch
        elif ch == ":":
            out.append((int(text[i + 1]), int(num)))
            num = ""
            i += 1
        else:
            out.append((OPS.index(ch), int(num)))
            num = ""
        i += 1
    return out


def rec(name=b"r", pos=100, cigar="", l_seq=None, qual=None, tags=b"", ref=0, flag=0, l_name=None, block_size=None):
    ops = cig(cigar) if isinstance(cigar, str) else cigar
    if qual is None:
        qual = bytes([30]) * (sum(n for o, n in ops if o in (0, 1, 4, 7, 8)) if l_seq is None else l_seq)
    if l_seq is None:
        l_seq = len(qual)
    nm = name + b"\0"
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(nm) if l_name is None else l_name, 60, 4680, len(ops), flag, l_seq, -1, -1, 0)
    body += nm + b"".join(struct.pack("<I", n << 4 | o) for o, n in ops) + bytes((l_seq + 1) // 2) + qual + tags
    return struct.pack("<i", len(body) if block_size is None else block_size) + body


def z(key, text, ty=b"Z"):
    return key + ty + text + b"\0"


def num(key, ty, v=1):
    return key + ty + struct.pack({b"c": "<b", b"C": "<B", b"s": "<h", b"S": "<H", b"i": "<i", b"I": "<I", b"f": "<f"}[ty], v)


def many_tags(n, dup=None):
    """n tags with distinct keys (X0..), `dup` = (i, j): tag j carries the key of tag i"""
    keys = [bytes([ord("a") + k // 62 % 26, b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"[k % 62]]) for k in range(n)]
    if dup:
        keys[dup[1]] = keys[dup[0]]
    return b"".join(num(k, b"C", i & 0xFF) for i, k in enumerate(keys))


def cases():
    c = []
    add = lambda label, r, m: c.append((label, r, m))
    # ---- names ----
    add("name len 1", rec(name=b"a"), OK)
    add("name len 254", rec(name=b"n" * 254), OK)
    add("name len 254 bad last", rec(name=b"n" * 253 + b" "), NAME_CHARS)
    add("name empty", rec(name=b""), NAME_EMPTY)
    for ch, m in ((0x20, NAME_CHARS), (0x21, OK), (0x40, NAME_CHARS), (0x7E, OK), (0x7F, NAME_CHARS)):
        add("name %02x first" % ch, rec(name=bytes([ch]) + b"bc"), m)
        add("name %02x middle" % ch, rec(name=b"a" + bytes([ch]) + b"c"), m)
        add("name %02x last" % ch, rec(name=b"ab" + bytes([ch])), m)
    # ---- positions ----
    add("pos -2", rec(pos=-2), POSITION)
    add("pos -1", rec(pos=-1), OK)
    add("pos 2^29-2", rec(pos=(1 << 29) - 2), OK)
    add("pos 2^29-1", rec(pos=(1 << 29) - 1), POSITION)
    # ---- qualities ----
    for n in (0, 1, 7, 8, 9, 63, 64, 65):
        add("qual %d all ff" % n, rec(qual=b"\xff" * n), OK)
        add("qual %d all 93" % n, rec(qual=b"\x5d" * n), OK)
        if n:
            add("qual %d one 94" % n, rec(qual=b"\x5d" * (n - 1) + b"\x5e"), QUALITIES)
            add("qual %d 94 first" % n, rec(qual=b"\x5e" + b"\x00" * (n - 1)), QUALITIES)
        if n > 1:
            add("qual %d ff then small first" % n, rec(qual=b"\x0a" + b"\xff" * (n - 1)), QUALITIES)
            add("qual %d ff then small last" % n, rec(qual=b"\xff" * (n - 1) + b"\x0a"), QUALITIES)
        if n > 8:
            add("qual %d small at the eighth byte" % n, rec(qual=b"\xff" * 7 + b"\x0a" + b"\xff" * (n - 8)), QUALITIES)
            add("qual %d 94 at the ninth byte" % n, rec(qual=b"\x00" * 8 + b"\x5e" + b"\x00" * (n - 9)), QUALITIES)
    add("qual ff ff 0a", rec(qual=b"\xff\xff\x0a"), QUALITIES)
    add("qual 5d", rec(qual=b"\x5d"), OK)
    add("qual 5e", rec(qual=b"\x5e"), QUALITIES)
    add("qual 80", rec(qual=b"\x80" * 16), QUALITIES)
    # ---- CIGAR ----
    add("cigar none, sequence", rec(cigar="", qual=b"\x10" * 5), OK)
    add("cigar 1", rec(cigar="5M"), OK)
    add("cigar HM", rec(cigar="2H5M"), OK)
    add("cigar SM", rec(cigar="2S5M"), OK)
    add("cigar SHM", rec(cigar="2S2H5M"), CIGAR_HARD)
    add("cigar HSM", rec(cigar="2H2S5M"), OK)
    add("cigar MSM", rec(cigar="3M2S5M"), CIGAR_SOFT)
    add("cigar MHM", rec(cigar="3M2H5M"), CIGAR_HARD)
    add("cigar HMSMH", rec(cigar="1H3M2S5M1H"), CIGAR_SOFT)
    add("cigar HSMSH", rec(cigar="1H2S5M2S1H"), OK)
    add("cigar SSM", rec(cigar="1S2S5M"), CIGAR_SOFT)
    add("cigar HSMS", rec(cigar="1H2S5M2S"), OK)
    add("cigar HHM", rec(cigar="1H1H5M"), CIGAR_HARD)
    add("cigar HMH", rec(cigar="1H5M1H"), OK)
    add("cigar MIDNM", rec(cigar="3M1I2D4N2M"), OK)
    add("cigar sum one short", rec(cigar="4M1I", l_seq=6, qual=b"\x10" * 6), CIGAR_LENGTH)
    add("cigar sum one long", rec(cigar="4M1I", l_seq=4, qual=b"\x10" * 4), CIGAR_LENGTH)
    add("cigar =X count", rec(cigar="2=3X"), OK)
    add("cigar D N H P do not count", rec(cigar="1H5M2D3N1P", l_seq=5), OK)
    add("cigar no sequence", rec(cigar="5M", l_seq=0, qual=b""), OK)
    add("cigar code 9", rec(cigar="5M2:9", l_seq=5, flag=4), OK)                # (flagged unmapped: tests/bamgen.py does not add up such a CIGAR)
    add("cigar code 9 counts nothing", rec(cigar="5M2:9", l_seq=7, qual=b"\x10" * 7, flag=4), CIGAR_LENGTH)
    add("cigar SHMHS and length", rec(cigar="1S1H5M1H1S", l_seq=9, qual=b"\x10" * 9), CIGAR_HARD | CIGAR_LENGTH)
    # ---- tags: the type rules ----
    add("H ok", rec(tags=z(b"XH", b"0aF9", b"H")), OK)
    add("H odd length", rec(tags=z(b"XH", b"0aF", b"H")), OK)
    add("H empty", rec(tags=z(b"XH", b"", b"H")), TAG_VALUE)
    add("H not hex", rec(tags=z(b"XH", b"0g", b"H")), TAG_VALUE)
    add("A !", rec(tags=b"XAA!"), OK)
    add("A ~", rec(tags=b"XAA~"), OK)
    add("A space", rec(tags=b"XAA "), TAG_VALUE)
    add("A 7f", rec(tags=b"XAA\x7f"), TAG_VALUE)
    add("Z ok with space", rec(tags=z(b"XZ", b"a b~")), OK)
    add("Z empty", rec(tags=z(b"XZ", b"")), TAG_VALUE)
    add("Z tab", rec(tags=z(b"XZ", b"a\tb")), TAG_VALUE)
    add("Z 7f", rec(tags=z(b"XZ", b"a\x7f")), TAG_VALUE)
    # ---- tags: predefined keys ----
    for ty in (b"c", b"C", b"s", b"S", b"i", b"I"):
        add("NM:" + ty.decode(), rec(tags=num(b"NM", ty)), OK)
    add("NM:f", rec(tags=num(b"NM", b"f", 1.0)), TAG_VALUE)
    add("NM:A", rec(tags=b"NMA1"), TAG_VALUE)
    add("NM:Z", rec(tags=z(b"NM", b"1")), TAG_VALUE)
    add("AS:i UQ:C", rec(tags=num(b"AS", b"i", -3) + num(b"UQ", b"C", 3)), OK)
    add("RG:Z", rec(tags=z(b"RG", b"grp1")), OK)
    add("RG:H", rec(tags=z(b"RG", b"ab", b"H")), TAG_VALUE)
    add("RG:i", rec(tags=num(b"RG", b"i")), TAG_VALUE)
    add("FZ:B:S", rec(tags=b"FZBS" + struct.pack("<IHH", 2, 1, 2)), OK)
    add("FZ:B:s", rec(tags=b"FZBs" + struct.pack("<Ihh", 2, 1, 2)), TAG_VALUE)
    add("FZ:Z", rec(tags=z(b"FZ", b"x")), TAG_VALUE)
    add("XB:B:f empty", rec(tags=b"XBBf" + struct.pack("<I", 0)), OK)
    add("OQ printable", rec(tags=z(b"OQ", b"!~II")), OK)
    add("OQ star", rec(tags=z(b"OQ", b"*")), OK)
    add("OQ space", rec(tags=z(b"OQ", b"I I")), TAG_VALUE)
    add("CQ Q2 U2 ok", rec(tags=z(b"CQ", b"II") + z(b"Q2", b"*") + z(b"U2", b"#")), OK)
    add("U2 space", rec(tags=z(b"U2", b" ")), TAG_VALUE)
    add("E2 l_seq", rec(cigar="5M", tags=z(b"E2", b"ACGTA")), OK)
    add("E2 l_seq - 1", rec(cigar="5M", tags=z(b"E2", b"ACGT")), TAG_VALUE)
    add("E2 l_seq + 1", rec(cigar="5M", tags=z(b"E2", b"ACGTAC")), TAG_VALUE)
    add("E2 star with l_seq 1", rec(cigar="1M", tags=z(b"E2", b"*")), OK)
    add("E2 star with l_seq 5", rec(cigar="5M", tags=z(b"E2", b"*")), TAG_VALUE)
    add("BQ l_seq", rec(cigar="5M", tags=z(b"BQ", b"@@ @@")), OK)
    add("BQ l_seq - 1", rec(cigar="5M", tags=z(b"BQ", b"@@@@")), TAG_VALUE)
    add("BQ l_seq + 1", rec(cigar="5M", tags=z(b"BQ", b"@@@@@@")), TAG_VALUE)
    for text, m in ((b"0", OK), (b"10A5", OK), (b"10^AC5", OK), (b"A5", TAG_VALUE), (b"10^5", TAG_VALUE), (b"10A", TAG_VALUE),
                    (b"10a5", TAG_VALUE), (b"^A1", TAG_VALUE), (b"10A5^G0T3", OK), (b"10AC5", TAG_VALUE), (b"5^", TAG_VALUE)):
        add("MD " + text.decode(), rec(tags=z(b"MD", text)), m)
    add("MD:i", rec(tags=num(b"MD", b"i")), TAG_VALUE)
    # ---- tags: duplicate keys ----
    add("2 tags distinct", rec(tags=many_tags(2)), OK)
    add("2 tags same", rec(tags=many_tags(2, (0, 1))), TAG_DUPLICATE)
    for n in (256, 257, 300):
        add("%d tags distinct" % n, rec(tags=many_tags(n)), OK)
        add("%d tags first + last" % n, rec(tags=many_tags(n, (0, n - 1))), TAG_DUPLICATE)
        add("%d tags last two" % n, rec(tags=many_tags(n, (n - 2, n - 1))), TAG_DUPLICATE)
    add("duplicate and bad value", rec(tags=z(b"XZ", b"") + num(b"XZ", b"i")), TAG_VALUE | TAG_DUPLICATE)
    add("one byte left over", rec(tags=num(b"XI", b"i") + b"Q"), OK)
    # ---- malformed ----
    add("block_size 31", struct.pack("<i", 31) + bytes(36), MALFORMED)
    add("block_size past the bytes", rec()[:-1], MALFORMED)
    add("l_read_name 0", rec(name=b"", l_name=0, pos=-5), MALFORMED)
    cut = rec(cigar="5M", pos=-5)[4:-1]                   # the last quality is missing, and block_size says so
    add("fixed part past block_size", struct.pack("<i", len(cut)) + cut, MALFORMED)
    add("negative l_seq", rec(l_seq=-1, qual=b"", pos=-5), MALFORMED)
    add("tag of unknown type", rec(pos=-2, tags=num(b"XI", b"i") + b"XQq\x01"), POSITION | MALFORMED)
    add("B of unknown element type", rec(tags=b"XBBA" + struct.pack("<I", 1) + b"x"), MALFORMED)
    add("B array past the record", rec(tags=b"XBBi" + struct.pack("<Ii", 2, 7)), MALFORMED)
    add("B array of 2^32 - 1", rec(tags=b"XBBi" + struct.pack("<I", 0xFFFFFFFF)), MALFORMED)
    add("B header cut", rec(tags=b"XBBi\x01\x00"), MALFORMED)
    add("value past the record", rec(tags=b"XIi\x01\x02"), MALFORMED)
    add("Z without NUL", rec(tags=b"XZZabc"), MALFORMED)
    add("H without NUL", rec(tags=b"XHH0a"), MALFORMED)
    add("key without type", rec(tags=num(b"XI", b"i") + b"XQ"), MALFORMED)
    add("bad tag, duplicate, then the break", rec(tags=z(b"XZ", b"") + num(b"XZ", b"c") + b"YYZno end"), TAG_VALUE | TAG_DUPLICATE | MALFORMED)
    add("bad tag behind the break is not judged", rec(tags=b"YYq\x01" + z(b"XZ", b"\t")), MALFORMED)
    return c


def stream_safe(r):
    """can the record stand in a BAM stream?  (its block_size is its length and is at least 32: the record chain holds)"""
    return len(r) >= 36 and struct.unpack_from("<i", r)[0] == len(r) - 4
