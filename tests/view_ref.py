"""Pure-Python restatement of the record selection of `sambamba view` (sambamba/view.d), the test oracle of the device path.

A record is selected when it passes the -F filter (a Python predicate here), --num-filter (FlagBitFilter, sambamba/utils/common/
filtering.d:176-187), the subsampling (SubsampleFilter, filtering.d:340-371) and the regions.  Regions listed on the command line
(view.d:339-361) give the concatenation, in listed order, of each region's records in file order -- "*" is the records with
ref_id < 0 --; a BED file (view.d:362-366, bed.d:37-55, 128-141) gives every record that overlaps one of the merged regions once.
Overlap is the predicate of BamReadFilter.findNext (BioD bio/std/hts/bam/randomaccessmanager.d:397-460) applied to every record.
The header is that of markdup: toSam of the input with the @PG line of addPG (utils/version_.d:9-22).
"""
import math
import struct

from tests.flagstat_ref import inflate
from tests.markdup_ref import header_text
from tests.sort_ref import split_stream

FNV_OFFSET, FNV_PRIME, M64 = 14695981039346656037, 1099511628211, (1 << 64) - 1
REF_CONSUMING = {0, 2, 3, 7, 8}         # M D N = X


def fields(rec):
    """(ref_id, pos, flag, mapq, name bytes, bases covered) of a record (block_size prefix included)."""
    ref, pos, l_name, mapq, _bin, n_cig, flag, _l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    name = rec[36:36 + max(l_name - 1, 0)]
    covered = 0
    if not flag & 0x4:                  # basesCovered (read.d:255-262): an unmapped read covers nothing
        for k in range(n_cig):
            c = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)[0]
            if c & 15 in REF_CONSUMING:
                covered += c >> 4
    return ref, pos, flag, mapq, name, covered


def overlaps(ref, pos, covered, region):
    """region: "*" or (ref_id, start, end)."""
    if region == "*":
        return ref < 0
    r, start, end = region
    return ref == r and pos < end and (pos > start or pos + covered > start)


def name_hash(name, seed):
    h = FNV_OFFSET
    for b in bytes(name) + struct.pack("<Q", seed):
        h = ((h ^ b) * FNV_PRIME) & M64
    return h


def threshold(fraction):
    """(0x100000000UL * fraction).to!ulong; None when the conversion throws."""
    t = 4294967296.0 * fraction
    if math.isnan(t) or t < 0 or t >= 2.0 ** 64:
        return None
    return int(t)


def subsample_keeps(name, fraction, seed):
    return (name_hash(name, seed) & 0xFFFFFFFF) < threshold(fraction)


def num_filter(text):
    """(bits_set, bits_unset) of --num-filter=text; None where to!ushort throws."""
    parts = text.split("/") if text else []
    out = [0, 0]
    for k, p in enumerate(parts[:2]):
        if p == "":
            continue
        if not (p.isascii() and p.isdigit()) or int(p) > 0xFFFF:
            return None
        out[k] = int(p)
    return tuple(out)


def flags_pass(flag, bits_set, bits_unset):
    return (flag & bits_set) == bits_set and (flag & bits_unset) == 0


JSON_ESCAPES = {8: "b", 9: "t", 10: "n", 12: "f", 13: "r", ord('"'): '"', ord("?"): "/", ord("\\"): "\\"}


def reference_info_json(refs):
    """outputReferenceInfoJson (view.d:98-118) for [(name, length)], as its code prints it: the quote in front of the brace; strings as
    writeStringJson escapes them (BioD bio/core/utils/format.d:214-248 -- the table has the solidus at '?')."""
    items = []
    for name, length in refs:
        s = "".join("\\" + JSON_ESCAPES[ord(c)] if ord(c) in JSON_ESCAPES else c for c in name)
        items.append('"{name":"%s","length":%d}' % (s, length))
    return "[" + ",".join(items) + "]\n"


def parse_region(text, refs):
    """"chr" / "chr:beg-end" -> (ref_id, start, end) against [(name, length)]; "*" stays "*" (region.d:97-246, view.d:348-356)."""
    if text == "*":
        return "*"
    name, beg, end = text, 0, None
    if ":" in text:
        head, tail = text.rsplit(":", 1)
        a, dash, b = tail.partition("-")
        num = lambda t: t != "" and all(c.isdigit() or c == "," for c in t) and any(c.isdigit() for c in t)
        if num(a) and (not dash or num(b)):
            name, beg = head, int(a.replace(",", "")) - 1
            end = int(b.replace(",", "")) if dash else None
    ids = [k for k, (n, _) in enumerate(refs) if n == name]
    if not ids:
        raise KeyError(name)
    return (ids[0], beg, refs[ids[0]][1] if end is None else end)


def merged_bed(lines, refs):
    """parseBed: [(ref_id, start, end)] sorted and merged (touching intervals too), names the BAM does not have dropped."""
    by = {}
    for line in lines:
        f = line.split()
        if len(f) < 2:
            continue
        beg = int(f[1])
        end = int(f[2]) if len(f) >= 3 else beg + 1
        if beg == end:
            end = beg + 1
        if beg < end:
            by.setdefault(f[0], []).append((beg, end))
    out = []
    for name, ivs in by.items():
        ids = [k for k, (n, _) in enumerate(refs) if n == name]
        if not ids:
            continue
        ivs.sort(key=lambda iv: iv[0])
        cur = list(ivs[0])
        for b, e in ivs[1:]:
            if cur[1] >= b:
                cur[1] = max(cur[1], e)
            else:
                out.append((ids[0], cur[0], cur[1]))
                cur = [b, e]
        out.append((ids[0], cur[0], cur[1]))
    return sorted(out)


def select(recs, keep=None, bits=None, subsample=None, regions=None, bed=None):
    """The selected records in output order.  keep(record) -> bool; bits = (set, unset); subsample = (fraction, seed); regions = the
    listed regions ("*" or (ref_id, start, end)); bed = the merged regions of a BED file."""
    def passes(rec):
        _, _, flag, _, name, _ = fields(rec)
        if keep is not None and not keep(rec):
            return False
        if bits is not None and not flags_pass(flag, *bits):
            return False
        return subsample is None or subsample_keeps(name, *subsample)

    kept = [r for r in recs if passes(r)]
    if regions:
        out = []
        for g in regions:
            out += [r for r in kept if overlaps(*(fields(r)[i] for i in (0, 1, 5)), g)]
        return out
    if bed is not None:
        return [r for r in kept if any(overlaps(*(fields(r)[i] for i in (0, 1, 5)), g) for g in bed)]
    return kept


def refs_of(stream):
    """[(name, length)] of the binary reference list."""
    _, refs, n_ref, _ = split_stream(stream)
    out, p = [], 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", refs, p)[0]
        out.append((refs[p + 4:p + 4 + l_name - 1].decode(), struct.unpack_from("<i", refs, p + 4 + l_name)[0]))
        p += 8 + l_name
    return out


def expected_stream(stream, command_line=None, **selection):
    """The inflated stream `view -f bam` writes for the inflated input `stream`; selection as select()."""
    text, refs, _, recs = split_stream(stream)
    new_text = header_text(text.decode(), command_line).encode()
    return b"BAM\1" + struct.pack("<i", len(new_text)) + new_text + refs + b"".join(select(recs, **selection))


def expected(path, command_line=None, **selection):
    return expected_stream(inflate(path), command_line, **selection)
