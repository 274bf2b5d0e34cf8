"""`sbx-subsample` restated in plain Python ("subsample"): the oracle of tests/test_gpu_subsample.py and of the
host checks, since the reference's subsample.d never drops a read.  A difference array per reference, FNV-1a over the read name, the
integer predicate.  Records are bytes with their block_size field, as tests/bamgen.py makes them and tests/sort_ref.py splits them."""
import struct

import numpy as np

from tests.flagstat_ref import inflate
from tests.sort_ref import split_stream

FNV_OFFSET, FNV_PRIME, M64 = 14695981039346656037, 1099511628211, (1 << 64) - 1
UNCOUNTED = 0x4 | 0x200 | 0x400
DROPPED = 0x200


def fnv1a64(data):
    h = FNV_OFFSET
    for b in bytes(data):
        h = ((h ^ b) * FNV_PRIME) & M64
    return h


def name_hash32(name):
    """low 32 bits of the 64-bit FNV-1a `view -s` uses: the name without its NUL, then the eight bytes of the seed 0"""
    return fnv1a64(bytes(name) + bytes(8)) & 0xFFFFFFFF


def name_of(rec):
    l_name = rec[12]
    return bytes(rec[36:36 + max(l_name - 1, 0)])


def flag_of(rec):
    return struct.unpack_from("<H", rec, 18)[0]


def bases_covered(rec):
    l_name = rec[12]
    n_cigar = struct.unpack_from("<H", rec, 16)[0]
    total = 0
    for k in range(n_cigar):
        op = struct.unpack_from("<I", rec, 36 + l_name + 4 * k)[0]
        if op & 15 in (0, 2, 3, 7, 8):
            total += op >> 4
    return total & 0xFFFFFFFF


def span(rec, lns):
    """None for a record that is not counted, else (ref_id, pos, e)"""
    ref, pos = struct.unpack_from("<ii", rec, 4)
    if flag_of(rec) & UNCOUNTED or not 0 <= ref < len(lns) or not 0 <= pos < lns[ref]:
        return None
    return ref, pos, min(pos + max(bases_covered(rec), 1), lns[ref])


def keeps(h, cov, max_cov):
    return cov <= max_cov or h * cov < (max_cov << 32)


def slot_bases(lns):
    base = [0]
    for ln in lns:
        base.append(base[-1] + max(ln, 0) + 1)
    return base


def coverage(recs, lns):
    """per reference the array c_r(p), p in [0, LN]: counted records with pos <= p < e (the entry at LN is 0)"""
    diff = [np.zeros(max(ln, 0) + 1, dtype=np.int64) for ln in lns]
    for rec in recs:
        s = span(rec, lns)
        if s:
            diff[s[0]][s[1]] += 1
            diff[s[0]][s[2]] -= 1
    return [np.cumsum(d) for d in diff]


def verdicts(recs, lns, max_cov):
    """per record (counted, cov, dropped); cov is 0 for a record that is not counted"""
    cov = coverage(recs, lns)
    out = []
    for rec in recs:
        s = span(rec, lns)
        if not s:
            out.append((False, 0, False))
            continue
        c = int(max(cov[s[0]][s[1]], cov[s[0]][s[2] - 1]))
        out.append((True, c, not keeps(name_hash32(name_of(rec)), c, max_cov)))
    return out


def subsample(recs, lns, max_cov, remove, tile=4096):
    """(records of the output, the counts sbx_subsample_stats reports); tile: subc::kCovTile, which cov_array_bytes is rounded up to"""
    v = verdicts(recs, lns, max_cov)
    out = []
    for rec, (_, _, dropped) in zip(recs, v):
        if not dropped:
            out.append(bytes(rec))
        elif not remove:
            r = bytearray(rec)
            struct.pack_into("<H", r, 18, flag_of(rec) | DROPPED)
            out.append(bytes(r))
    stats = {"n_records": len(recs), "n_counted": sum(c for c, _, _ in v), "n_over": sum(c and cov > max_cov for c, cov, _ in v),
             "n_dropped": sum(d for _, _, d in v), "n_written": len(out), "max_cov_seen": max([cov for _, cov, _ in v] + [0]),
             "cov_array_bytes": -(-slot_bases(lns)[-1] // tile) * tile * 4}
    return out, stats


def read_bam(path):
    """(header text, [LN], [record bytes]) of a BAM file"""
    text, refs, n_ref, recs = split_stream(bytes(inflate(path)))
    lns, p = [], 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", refs, p)[0]
        lns.append(struct.unpack_from("<i", refs, p + 4 + l_name)[0])
        p += 8 + l_name
    return text.decode(), lns, recs
