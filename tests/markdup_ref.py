"""Pure-Python restatement of `sambamba markdup` (sambamba/markdup.d), the test oracle of the device path.

Records with a reference id that are not unmapped, secondary or supplementary take part.  Each yields (library, ref_id, 5' coordinate
after unclipping, strand, score = sum of the base qualities >= 15); `paired` is flag 1 without flag 8.  Paired records are matched by
(read name, RG string) -- 1st with 2nd, 3rd with 4th occurrence in file order, a leftover is an unmatched single end (the reference's
outcome for a key that does not occur exactly twice depends on its hash table; this is the project's definition).  Pairs are grouped
by pairedEndsInfoComparator's fields, single ends by singleEndInfoComparator's; the best of a group has the highest score and, among
equals, comes first in the file (the reference's choice among equals depends on an unstable sort).  expected_stream() is the INFLATED
output: "BAM\\1", l_text, text, reference list, records in input order with flag 0x400 set / cleared.
"""
import struct

from tests import sort_ref
from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream

KNOWN_SO = ("unsorted", "coordinate", "queryname")


def _parse(text):
    """(version, SO, {type: ordered {id: serialised line}}, [LB per kept @RG], comments) as SamHeader's constructor reads the text."""
    text = text.split("\0")[0]
    version, so, first = "1.3", "", True
    dicts = {"SQ": ({}, sort_ref.SQ_FIELDS), "RG": ({}, sort_ref.RG_FIELDS), "PG": ({}, sort_ref.PG_FIELDS)}
    libraries, comments = [], []
    for line in text.split("\n"):
        if len(line) < 3:
            continue
        if first and line[:3] == "@HD":
            version = sort_ref._fields(line).get("VN", "")
            so = sort_ref._fields(line).get("SO", "")
        assert line[0] == "@"
        ty = line[1:3]
        if ty in dicts:
            seen, order = dicts[ty]
            ident, out = sort_ref._serialise("@" + ty, order, line)
            if ident not in seen:
                seen[ident] = out
                if ty == "RG":
                    libraries.append(sort_ref._fields(line).get("LB", ""))
        elif ty == "CO":
            comments.append(line[4:])
        else:
            assert ty == "HD", line
        first = False
    return version, so, dicts, libraries, comments


def header_text(text, command_line):
    """The header text of the output for the input's header text (str); command_line is the CL of the added @PG (None: none added)."""
    version, so, dicts, _, comments = _parse(text)
    pg = dicts["PG"][0]
    if command_line is not None and "sambamba" not in pg:
        line = "@PG\tID:sambamba"
        if command_line:
            line += "\tCL:" + command_line
        if pg and list(pg)[-1]:
            line += "\tPP:" + list(pg)[-1]
        pg["sambamba"] = line + "\tVN:1.0"
    lines = ["@HD\tVN:%s%s" % (version, "\tSO:" + so if so in KNOWN_SO else "")]
    for ty in ("SQ", "RG", "PG"):
        lines += list(dicts[ty][0].values())
    lines += ["@CO\t" + c for c in comments]
    return "".join(x + "\n" for x in lines)


def library_ids(text):
    """{read group id: library id} (ReadGroupIndex, markdup.d:659-696): libraries are numbered by first appearance of the LB string."""
    _, _, dicts, libraries, _ = _parse(text)
    libs, out = {}, {}
    for ident, lb in zip(dicts["RG"][0], libraries):
        out[ident] = libs.setdefault(lb, len(libs))
    return out


def _s32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v


def five_prime_coord(pos, reverse, cigar):
    """computeFivePrimeCoord; cigar: [(op character, length)]."""
    if not reverse:
        clip = 0
        for op, n in cigar:
            if op not in "SH":
                break
            clip += n
        return _s32(pos - clip)
    clip = 0
    for op, n in reversed(cigar):
        if op not in "SH":
            break
        clip += n
    return _s32(pos + sum(n for op, n in cigar if op in "MDN=X") + clip)


def score(quals):
    return sum(q for q in quals if q >= 15) & 0xFFFFFFFF


def rg_of(rec, tags_at):
    """The RG:Z string among the aux fields of a record, or None."""
    p, e = tags_at, len(rec)
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while p + 3 <= e:
        key, ty = rec[p:p + 2], chr(rec[p + 2])
        p += 3
        if ty in size:
            q = p + size[ty]
        elif ty in "ZH":
            q = rec.index(b"\0", p) + 1
        elif ty == "B":
            sub, n = chr(rec[p]), struct.unpack_from("<I", rec, p + 1)[0]
            q = p + 5 + n * (1 if sub in "cC" else 2 if sub in "sS" else 4)
        else:
            return None
        if key == b"RG":
            return rec[p:q - 1] if ty == "Z" else None
        p = q
    return None


def describe(rec, libs):
    """None for a record that does not take part, else a dict with the fields of SingleEndInfo plus the pairing key."""
    ref, pos, l_name, _mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    if ref == -1 or flag & 0x904:
        return None
    p = 36 + l_name
    cigar = []
    for k in range(n_cig):
        c = struct.unpack_from("<I", rec, p + 4 * k)[0]
        cigar.append(("MIDNSHP=X"[c & 15] if (c & 15) < 9 else "?", c >> 4))
    p += 4 * n_cig + (l_seq + 1) // 2
    quals = rec[p:p + l_seq]
    rg = rg_of(rec, p + l_seq)
    reverse = 1 if flag & 0x10 else 0
    lib = libs.get(rg.decode("latin-1"), -1) if rg is not None else -1
    return {"library": lib, "ref": ref, "coord": five_prime_coord(pos, reverse, cigar), "reversed": reverse, "score": score(quals),
            "paired": bool(flag & 1) and not flag & 8, "key": (rec[36:36 + l_name], rg or b"")}


def single_key(e):
    """singleEndInfoComparator's fields."""
    return (e["library"], e["ref"], e["coord"], e["reversed"])


def single_end_before(a, b):
    """singleEndInfoComparator (markdup.d:615-624) on (library, ref_id, coord, reversed)."""
    return tuple(a) < tuple(b)


def paired_ends_before(a, b):
    """pairedEndsInfoComparator (markdup.d:626-641) on (library, ref1, coord1, reversed1, reversed2, ref2, coord2)."""
    return tuple(a) < tuple(b)


def combine(e1, e2):
    """markdup.d:731-753: (library, ref1, coord1, reversed1, reversed2, ref2, coord2), end1 key, end2 key, score; e1 is the earlier record."""
    if (e2["ref"], e2["coord"], e2["reversed"]) < (e1["ref"], e1["coord"], e1["reversed"]):
        e1, e2 = e2, e1
    key = (e1["library"], e1["ref"], e1["coord"], e1["reversed"], e2["reversed"], e2["ref"], e2["coord"])
    return key, single_key(e1), single_key(e2), (e1["score"] + e2["score"]) & 0xFFFFFFFF


def analyse(records, text):
    """(duplicate indices, n_end_pairs, n_single_ends, n_unmatched_pairs)"""
    libs = library_ids(text)
    ends = [describe(r, libs) for r in records]
    waiting, pairs, singles = {}, [], []
    for i, e in enumerate(ends):
        if e is None:
            continue
        if not e["paired"]:
            singles.append(i)
        elif e["key"] in waiting:
            pairs.append((waiting.pop(e["key"]), i))
        else:
            waiting[e["key"]] = i
    unmatched = sorted(waiting.values())
    singles = sorted(singles + unmatched)
    dup = set()
    groups, seen_paired = {}, set()
    for i, j in pairs:
        key, k1, k2, sc = combine(ends[i], ends[j])
        groups.setdefault(key, []).append((-sc, i, j))
        seen_paired.update((k1, k2))
    for members in groups.values():
        for _, i, j in sorted(members)[1:]:
            dup.update((i, j))
    for i in unmatched:
        seen_paired.add(single_key(ends[i]))
    frags = {}
    for i in singles:
        if not ends[i]["paired"]:
            frags.setdefault(single_key(ends[i]), []).append((-ends[i]["score"], i))
    for key, members in frags.items():
        members = sorted(members)
        dup.update(i for _, i in (members if key in seen_paired else members[1:]))
    return dup, len(pairs), len(singles), len(unmatched)


def duplicates(records, text=""):
    """The indices of the records `sambamba markdup` marks; text is the SAM header text (read groups -> libraries)."""
    return analyse(records, text)[0]


def output_flag(flag, marked):
    if marked:
        return flag | 0x400
    return flag if flag & 0x900 else flag & ~0x400


def expected_stream(stream, remove=False, command_line=None):
    """The inflated stream `sambamba markdup` writes for the inflated input `stream`."""
    text, refs, _, recs = split_stream(stream)
    dup = duplicates(recs, text.decode())
    out = []
    for i, r in enumerate(recs):
        flag = output_flag(struct.unpack_from("<H", r, 18)[0], i in dup)
        if remove and flag & 0x400:
            continue
        out.append(r[:18] + struct.pack("<H", flag) + r[20:])
    new_text = header_text(text.decode(), command_line).encode()
    return b"BAM\1" + struct.pack("<i", len(new_text)) + new_text + refs + b"".join(out)


def expected(path, remove=False, command_line=None):
    return expected_stream(inflate(path), remove, command_line)
