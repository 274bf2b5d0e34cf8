"""Pure-Python restatement of `sambamba merge` for coordinate-sorted inputs (sambamba/merge.d, BioD
bio/std/hts/utils/samheadermerger.d), the test oracle of sbx_merge_bam.  It works on inflated streams.

Headers (SamHeaderMerger): the sorting orders must agree; the @SQ dictionaries are merged in the topological order of "line k comes
before line k + 1 of its file" (utils/graph.d: Kahn's algorithm, FIFO queue seeded in node order, successors in edge order), with all
lines sorted by name when the files contradict one another; @RG and @PG lines with one id and the same fields are one line, a line
whose id a different line has taken is renamed id.1, id.2, ...; @PG lines are merged level by level from the lines without PP, a
child's PP rewritten through its own file's map first; @CO lines are concatenated.  Where the reference iterates D associative arrays
the order is defined: inputs in order, lines in order of appearance, the first line to claim an id keeps it.

Records (merge.d:133-207 `modifier`): ref_id -- and, unlike the reference, next_ref_id too -- goes through the input's map, the value of
the first RG:Z and of the first PG:Z aux field is replaced when the map renames it, block_size follows.  The output is the stable sort
(sort_ref.record_key) of the rewritten records of input 1, input 2, ...: ties come out lower input first, then in file order.
"""
import struct

from tests import sort_ref
from tests.sort_ref import PG_FIELDS, RG_FIELDS, SQ_FIELDS, _fields, _serialise, record_key, split_stream


class MergeError(Exception):
    pass


def _parse(text):
    """(SO, {SQ, RG, PG: [(id, serialised line)]}, comments) as SamHeader reads a text."""
    text = text.split("\0")[0]
    so, first = "", True
    dicts = {"SQ": ({}, SQ_FIELDS), "RG": ({}, RG_FIELDS), "PG": ({}, PG_FIELDS)}
    comments = []
    for line in text.split("\n"):
        if len(line) < 3:
            continue
        if first and line[:3] == "@HD":
            so = _fields(line).get("SO", "")
        ty = line[1:3]
        if ty in dicts:
            seen, order = dicts[ty]
            ident, out = _serialise("@" + ty, order, line)
            seen.setdefault(ident, out)
        elif ty == "CO":
            comments.append(line[4:])
        first = False
    return so, {ty: list(d[0].items()) for ty, d in dicts.items()}, comments


def _with_field(line, key, value):
    parts = line.split("\t")
    for k in range(1, len(parts)):
        if parts[k][:3] == key + ":":
            parts[k] = key + ":" + value
            return "\t".join(parts)
    return "\t".join(parts[:1] + [key + ":" + value] + parts[1:])


def _merge_dictionaries(dicts):
    """dicts: per file [(name, length)] -> (merged [(name, length)], per file [new id])."""
    nodes, index, edges = [], {}, []

    def node(name, length):
        if name in index:
            if nodes[index[name]][1] != length:
                raise MergeError("can't merge SAM headers: one of references with name %s has length %d while another one with the same "
                                 "name has length %d" % (name, nodes[index[name]][1], length))
            return index[name]
        index[name] = len(nodes)
        nodes.append((name, length))
        edges.append([])
        return index[name]

    for d in dicts:
        prev = None
        for name, length in d:
            cur = node(name, length)
            if prev is not None:
                edges[prev].append(cur)
            prev = cur
    pred = [0] * len(nodes)
    for e in edges:
        for v in e:
            pred[v] += 1
    queue = [v for v in range(len(nodes)) if not pred[v]]
    head = 0
    while head < len(queue):
        for w in edges[queue[head]]:
            pred[w] -= 1
            if not pred[w]:
                queue.append(w)
        head += 1
    if len(queue) == len(nodes):
        merged = [nodes[v] for v in queue]
    else:                                               # a cycle: all lines sorted by name, in byte order
        merged = sorted(nodes, key=lambda r: r[0].encode())
    new_id = {name: k for k, (name, _) in enumerate(merged)}
    return merged, [[new_id[name] for name, _ in d] for d in dicts]


def _merge_lines(lines, taken, out, maps):
    """lines: [(file, id, text)] in the defined order; mergeHeaderLines."""
    seen = {}
    for f, ident, text in lines:
        if (ident, text) not in seen:
            new_id, k = ident, 0
            while new_id in taken:
                k += 1
                new_id = "%s.%d" % (ident, k)
            taken.add(new_id)
            out.append(text if new_id == ident else _with_field(text, "ID", new_id))
            seen[(ident, text)] = new_id
        maps[f].setdefault(ident, seen[(ident, text)])


def merge_headers(texts):
    """-> (merged text, merged [(name, length)], per input {"ref": [new id], "rg": {old: new}, "pg": {old: new}})."""
    parsed = [_parse(t) for t in texts]
    expected = parsed[0][0]
    if expected not in ("coordinate", "queryname"):
        raise MergeError("file headers indicate that some files are not sorted")
    if any(p[0] != expected for p in parsed):
        raise MergeError("sorting orders of files don't agree, can't merge")
    n = len(texts)
    dicts = [[(ident, int(_fields(line).get("LN", "0"))) for ident, line in p[1]["SQ"]] for p in parsed]
    merged, ref_maps = _merge_dictionaries(dicts)
    first_line = {}
    for p in parsed:
        for ident, line in p[1]["SQ"]:
            first_line.setdefault(ident, line)
    out = ["@HD\tVN:1.3\tSO:coordinate"] + [first_line[name] for name, _ in merged]
    # @RG
    rg_maps, rg_out = [dict() for _ in range(n)], []
    _merge_lines([(f, ident, line) for f, p in enumerate(parsed) for ident, line in p[1]["RG"]], set(), rg_out, rg_maps)
    # @PG, level by level
    pg_maps, pg_out, taken = [dict() for _ in range(n)], [], set()
    every = [(f, ident, _fields(line).get("PP", ""), line) for f, p in enumerate(parsed) for ident, line in p[1]["PG"]]
    done = set()
    level = [k for k, e in enumerate(every) if e[2] == ""]
    while level:
        lines = []
        for k in level:
            f, ident, pp, line = every[k]
            done.add(k)
            if pp and pg_maps[f].get(pp, pp) != pp:
                line = _with_field(line, "PP", pg_maps[f][pp])
            lines.append((f, ident, line))
        _merge_lines(lines, taken, pg_out, pg_maps)
        parents = {(every[k][0], every[k][1]) for k in level}
        level = [k for k, e in enumerate(every) if k not in done and e[2] != "" and (e[0], e[2]) in parents]
    out += rg_out + pg_out
    for p in parsed:
        out += ["@CO\t" + c for c in p[2]]
    maps = [{"ref": ref_maps[f], "rg": rg_maps[f], "pg": pg_maps[f]} for f in range(n)]
    return "".join(x + "\n" for x in out), merged, maps


AUX_SIZE = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_fields(rec):
    """[(tag, type, offset of the value, offset behind the field)] of a record (block_size included)."""
    ref, pos, l_name, mapq, _bin, n_cigar, flag, l_seq = struct.unpack_from("<iiBBHHHi", rec, 4)
    t = 36 + l_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
    out = []
    while t < len(rec):
        tag, ty = rec[t:t + 2], chr(rec[t + 2])
        v = t + 3
        if ty in AUX_SIZE:
            e = v + AUX_SIZE[ty]
        elif ty in "ZH":
            e = rec.index(b"\0", v) + 1
        else:
            assert ty == "B", ty
            e = v + 5 + struct.unpack_from("<I", rec, v + 1)[0] * AUX_SIZE[chr(rec[v])]
        out.append((tag, ty, v, e))
        t = e
    assert t == len(rec)
    return out


def rewrite_record(rec, m):
    ref, = struct.unpack_from("<i", rec, 4)
    nxt, = struct.unpack_from("<i", rec, 24)
    n_own = len(m["ref"])
    body = bytearray(rec[4:])
    if 0 <= ref < n_own:
        struct.pack_into("<i", body, 0, m["ref"][ref])
    if 0 <= nxt < n_own:
        struct.pack_into("<i", body, 20, m["ref"][nxt])
    out, at, seen = bytearray(), 0, set()
    for tag, ty, v, e in aux_fields(rec):
        if ty != "Z" or tag not in (b"RG", b"PG") or tag in seen:
            continue
        seen.add(tag)
        old = rec[v:e - 1].decode("latin-1")
        new = m["rg" if tag == b"RG" else "pg"].get(old, old)
        if new != old:
            out += body[at:v - 4] + new.encode("latin-1")
            at = e - 1 - 4
    out += body[at:]
    return struct.pack("<i", len(out)) + bytes(out)


def expected_stream(streams, keep=None):
    """The inflated stream sbx_merge_bam writes for the inflated inputs; keep(record bytes of the input) -> bool is the filter."""
    parts = [split_stream(s) for s in streams]
    text, refs, maps = merge_headers([p[0].decode() for p in parts])
    recs = []
    for p, m in zip(parts, maps):
        recs += [rewrite_record(r, m) for r in p[3] if keep is None or keep(r)]
    recs = sorted(recs, key=lambda r: record_key(r, len(refs)))
    ref_bytes = struct.pack("<i", len(refs))
    for name, length in refs:
        ref_bytes += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", length)
    return b"BAM\1" + struct.pack("<i", len(text)) + text.encode() + ref_bytes + b"".join(recs)


def expected(paths, keep=None):
    return expected_stream([sort_ref.inflate(p) for p in paths], keep)
