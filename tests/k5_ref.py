"""The three closed forms at the head of sambamba_amd/csrc/reduce.hip, restated in plain Python on exact integers, from the records
alone (tests/test_k5_cases_cpu.py compares them with the oracle's text, tests/test_gpu_k5_edges.py the device with them):

    n_bases[r]      = number of M/=/X bases at positions of r with quality >= min_bq, the CIGAR's lengths as written
                      (countOverlappingBases, sambamba/depth.d:671-698)
    n_reads[r]      = number of admitted reads with at least one such base inside r
    cov_count[r][t] = number of positions p of r with COV(p) >= T_t; COV(p) = the reads of the pileup column at p whose base there has
                      quality >= min_bq, a deletion or skip counting as quality 255.  The column walk is the pileup's
                      (pileup.d:175-222): an operation of length zero that consumes reference still takes one column, and the
                      read leaves the pileup at position + (sum of the reference lengths as written).
    seen[r]         = a pileup column exists inside r.

A read is admitted under the default filter (mapping quality > 0, not duplicate, not failed QC), when it is not flagged unmapped
and covers at least one reference position.  `format_*` print the numbers as `depth region` / `depth window` do (depth.d:847-876)."""
import struct

import numpy as np

from tests import bamgen as bg

REF_OPS, QUERY_OPS, MATCH_OPS = "MDN=X", "MIS=X", "M=X"


def parse(b, group_ids=()):
    ref, pos, l_name, mapq, _bin, n_cig, flag, l_seq = struct.unpack_from("<iiBBHHHi", b, 4)
    at = 36 + l_name
    cig = [struct.unpack_from("<I", b, at + 4 * i)[0] for i in range(n_cig)]
    at += 4 * n_cig + (l_seq + 1) // 2
    qual = list(b[at:at + l_seq])
    tags = bytes(b[at + l_seq:])
    sample = 0
    if group_ids and tags[:3] == b"RGZ":
        sample = group_ids.index(tags[3:tags.index(b"\0", 3)].decode())
    return {"ref": ref, "pos": pos, "mapq": mapq, "flag": flag, "qual": qual, "sample": sample,
            "cigar": [(bg.CIGAR_OPS[c & 15], c >> 4) for c in cig]}


def span(r):
    return sum(n for op, n in r["cigar"] if op in REF_OPS)


def admitted(r):
    return not r["flag"] & (0x4 | 0x200 | 0x400) and r["mapq"] > 0 and span(r) > 0


def bases_as_written(r):
    """[(reference position, quality)] of the M/=/X bases, the lengths of the CIGAR as written."""
    out, rp, qp = [], r["pos"], 0
    for op, n in r["cigar"]:
        if op in MATCH_OPS:
            out += [(rp + k, r["qual"][qp + k]) for k in range(min(n, len(r["qual"]) - qp))]
        if op in REF_OPS:
            rp += n
        if op in QUERY_OPS:
            qp += n
    return out


def columns(r):
    """[(reference position, quality of the read in the pileup column there)]: the cursor of pileup.d, 255 off a match."""
    cig, out = r["cigar"], []
    i = qoff = off = 0

    def skip_to_ref(i, qoff):
        while i < len(cig) and cig[i][0] not in REF_OPS:
            if cig[i][0] in QUERY_OPS:
                qoff += cig[i][1]
            i += 1
        return i, qoff

    i, qoff = skip_to_ref(0, 0)
    for p in range(r["pos"], r["pos"] + span(r)):
        op, n = cig[i]
        out.append((p, r["qual"][qoff] if op in MATCH_OPS else 255))
        off += 1
        if op in QUERY_OPS:
            qoff += 1
        if off >= n:
            off = 0
            i, qoff = skip_to_ref(i + 1, qoff)
    return out


class Restatement:
    """Per contig and sample: good[p] (bases counted at p), cov[p] (COV), col[p] (a column exists), and per read the sorted positions
    of its good bases.  `combined`: one sample."""
    def __init__(self, case, min_bq, combined=False):
        self.S = 1 if combined else case.n_samples
        self.refs = case.refs
        groups = [g for g, _ in case.read_groups]
        reads = [parse(b, groups) for b in case.records]
        self.reads = [r for r in reads if admitted(r)]
        reach = [ln for _, ln in case.refs]
        for ref, a, b in tuple(case.bed) + tuple(case.api_ranges):
            reach[ref] = max(reach[ref], a, b)
        for r in self.reads:
            reach[r["ref"]] = max(reach[r["ref"]], r["pos"] + span(r))
        self.good = [np.zeros((self.S, n + 1), dtype=np.int64) for n in reach]
        self.cov = [np.zeros((self.S, n + 1), dtype=np.int64) for n in reach]
        self.col = [np.zeros(n + 1, dtype=np.int64) for n in reach]
        self.good_at = []                   # per admitted read: (ref, sample, sorted positions of its good bases)
        for r in self.reads:
            s = 0 if combined else r["sample"]
            g = [p for p, q in bases_as_written(r) if q >= min_bq]
            for p in g:
                self.good[r["ref"]][s, p] += 1
            self.good_at.append((r["ref"], s, np.array(sorted(g), dtype=np.int64)))
            for p, q in columns(r):
                self.col[r["ref"]][p] = 1
                if q >= min_bq:
                    self.cov[r["ref"]][s, p] += 1

    def stats(self, ranges, thresholds=()):
        """(n_reads[n][S], n_bases[n][S], cov[n][S][n_thr], seen[n]) of ranges [(ref, start, end)], end < start read as empty."""
        n, S = len(ranges), self.S
        ranges = [(r, a, max(a, b)) for r, a, b in ranges]
        n_reads, n_bases = np.zeros((n, S), dtype=np.int64), np.zeros((n, S), dtype=np.int64)
        cov, seen = np.zeros((n, S, len(thresholds)), dtype=np.int64), np.zeros(n, dtype=np.int64)
        for ref in range(len(self.refs)):
            ids = [i for i, g in enumerate(ranges) if g[0] == ref]
            if not ids:
                continue
            a, b = np.array([ranges[i][1] for i in ids]), np.array([ranges[i][2] for i in ids])
            zero = np.zeros((S, 1), dtype=np.int64)
            gsum = np.concatenate([zero, np.cumsum(self.good[ref], axis=1)], axis=1)
            n_bases[ids] = (gsum[:, b] - gsum[:, a]).T
            csum = np.concatenate([[0], np.cumsum(self.col[ref])])
            seen[ids] = csum[b] > csum[a]
            for t, thr in enumerate(thresholds):
                tsum = np.concatenate([zero, np.cumsum(self.cov[ref] >= thr, axis=1)], axis=1)
                cov[ids, :, t] = (tsum[:, b] - tsum[:, a]).T
            for rref, s, g in self.good_at:
                if rref == ref and len(g):
                    hit = np.searchsorted(g, a) < np.searchsorted(g, b)
                    n_reads[np.array(ids)[hit], s] += 1
        return n_reads, n_bases, cov, seen

    def windows(self, ref, w):
        return [(ref, k * w, (k + 1) * w) for k in range(self.refs[ref][1] // w)]


def _g(x):
    return "%g" % float(x)


def _rows(lines, ranges, n_reads, n_bases, cov, thresholds, names):
    out = []
    for i, (line, (_, a, b)) in enumerate(zip(lines, ranges)):
        length = np.float32(b - a)
        for s in range(n_reads.shape[1]):
            row = [line, str(int(n_reads[i, s]) & 0xFFFFFFFF), _g(np.float32(int(n_bases[i, s]) & 0xFFFFFFFF) / length)]
            row += ["100" if thr == 0 else _g(np.float32(cov[i, s, t]) * np.float32(100) / length) for t, thr in enumerate(thresholds)]
            out.append("\t".join(row + ([names[s]] if names else [])) + "\n")
    return out


def _header(thresholds, names):
    return ("# chrom\tchromStart\tchromEnd\treadCount\tmeanCoverage" + "".join("\tpercentage%d" % t for t in thresholds) +
            ("\tsampleName" if names else "") + "\n")


def _names(case, combined):
    return None if combined else [s for _, s in case.read_groups] or ["*"]


def format_region(case, rs, thresholds=(), combined=False):
    """The text of `depth region -L <the case's BED file>` (no -c / -C / -a: every row is printed)."""
    names = _names(case, combined)
    lines = ["%s\t%d\t%d" % (case.refs[r][0], a, b) for r, a, b in case.bed]
    n_reads, n_bases, cov, _ = rs.stats(case.bed, thresholds)
    return (_header(thresholds, names) + "".join(_rows(lines, case.bed, n_reads, n_bases, cov, thresholds, names))).encode()


def format_window(case, rs, w, thresholds=(), combined=False):
    """The text of `depth window -w <w>`: every full window of every contig, those of a contig without a read included -- but none
    that ends at or before the first pileup column of the file: the reference creates its per-sample data at the first column
    (sampleData, depth.d:984-991) and printWindowStats loops over the samples it has, so the windows it finishes on the way there
    print no row (the contigs in front of the first read's, and the windows of that contig in front of the read)."""
    names = _names(case, combined)
    first = min(((r["ref"], r["pos"]) for r in rs.reads), default=(len(case.refs), 0))
    ranges = [g for ref in range(len(case.refs)) for g in rs.windows(ref, w) if (g[0], g[2]) > first]
    lines = ["%s\t%d\t%d" % (case.refs[r][0], a, b) for r, a, b in ranges]
    n_reads, n_bases, cov, _ = rs.stats(ranges, thresholds)
    return (_header(thresholds, names) + "".join(_rows(lines, ranges, n_reads, n_bases, cov, thresholds, names))).encode()
