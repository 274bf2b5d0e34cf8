"""Pure-Python restatement of `sambamba sort` in coordinate order (sambamba/sort.d, default mode), the test oracle of the device path.

Order: compareCoordinatesAndStrand (BioD bio/std/hts/bam/read.d:1632-1642) applied by a stable sort -- ref_id -1 last, ascending
ref_id, ascending position as a signed number, forward strand in front of reverse strand, ties in file order (records with ref_id -1
are all ties, whatever their position and strand); Python's sorted() is stable.  Header: the text is re-serialised as SamHeader.toSam prints it (BioD bio/std/hts/sam/header.d:216-254, 473-545, 626-656) after
sort.d:294-298 set the sorting order; the binary reference list is the input's.  expected_stream() is the INFLATED output: "BAM\\1",
l_text, text, reference list, records.
"""
import struct

from tests.flagstat_ref import inflate

SQ_FIELDS = ("SN", "LN", "AN", "AS", "DS", "M5", "SP", "UR", "AH")
RG_FIELDS = ("ID", "BC", "CN", "DS", "DT", "FO", "KS", "LB", "PG", "PI", "PL", "PU", "SM", "PM")
PG_FIELDS = ("ID", "PN", "CL", "PP", "VN")
NUMERIC = {"LN", "PI"}


def _fields(line):
    """{abbreviation: contents} of a header line; a field that comes twice keeps its last value."""
    out = {}
    for f in line[3:].split("\t"):
        if len(f) >= 3 and f[2] == ":":
            out[f[:2]] = f[3:]
    return out


def _serialise(prefix, order, line):
    got = _fields(line)
    text, ident = prefix, None
    for k, key in enumerate(order):
        v = got.get(key, "")
        if key in NUMERIC and v != "":
            v = "" if int(v) == 0 else str(int(v))
        if k == 0:
            ident = v
        if v != "":
            text += "\t%s:%s" % (key, v)
    return ident, text


def header_text(text):
    """The header text of the sorted file for the input's header text (str)."""
    text = text.split("\0")[0]
    version, first = "1.3", True
    dicts = {"SQ": ({}, SQ_FIELDS), "RG": ({}, RG_FIELDS), "PG": ({}, PG_FIELDS)}
    comments = []
    for line in text.split("\n"):
        if len(line) < 3:
            continue
        if first and line[:3] == "@HD":
            version = _fields(line).get("VN", "")
        assert line[0] == "@"
        ty = line[1:3]
        if ty in dicts:
            seen, order = dicts[ty]
            ident, out = _serialise("@" + ty, order, line)
            seen.setdefault(ident, out)                 # insertion-ordered; the first line with an id stays
        elif ty == "CO":
            comments.append(line[4:])
        else:
            assert ty == "HD", line
        first = False
    lines = ["@HD\tVN:%s\tSO:coordinate" % version]
    for ty in ("SQ", "RG", "PG"):
        lines += list(dicts[ty][0].values())
    lines += ["@CO\t" + c for c in comments]
    return "".join(x + "\n" for x in lines)


def split_stream(stream):
    """(header text bytes, reference list bytes incl. n_ref, n_ref, [record bytes incl. block_size]) of an inflated BAM stream."""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text]
    p = 8 + l_text
    r0 = p
    n_ref = struct.unpack_from("<i", stream, p)[0]
    p += 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, p)[0]
        p += 8 + l_name
    refs = stream[r0:p]
    recs = []
    while p < len(stream):
        bs = struct.unpack_from("<i", stream, p)[0]
        recs.append(stream[p:p + 4 + bs])
        p += 4 + bs
    assert p == len(stream)
    return text, refs, n_ref, recs


def before(a, b, n_ref=None):
    """compareCoordinatesAndStrand on (ref_id, position, strand) triples: does a come strictly before b?"""
    (ra, pa, sa), (rb, pb, sb) = a, b
    if ra == -1:
        return False
    if rb == -1:
        return True
    if ra != rb:
        return ra < rb
    if pa != pb:
        return pa < pb
    return (not sa) and sb


def record_key(rec, n_ref):
    ref, pos = struct.unpack_from("<ii", rec, 4)
    flag = struct.unpack_from("<I", rec, 16)[0] >> 16
    if ref < 0:
        return (n_ref, 0, 0)            # read.d:1635-1636: neither of two such records is before the other
    return (ref, pos, 1 if flag & 0x10 else 0)


def expected_stream(stream, keep=None):
    """The inflated stream `sambamba sort` writes for the inflated input `stream`; keep(record bytes) -> bool is the filter."""
    text, refs, n_ref, recs = split_stream(stream)
    if keep is not None:
        recs = [r for r in recs if keep(r)]
    recs = sorted(recs, key=lambda r: record_key(r, n_ref))
    new_text = header_text(text.decode()).encode()
    return b"BAM\1" + struct.pack("<i", len(new_text)) + new_text + refs + b"".join(recs)


def expected(path, keep=None):
    return expected_stream(inflate(path), keep)
