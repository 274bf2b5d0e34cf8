"""The definition of `sbx-slice` restated in Python, from the header comment of sambamba/slice.d (test harness only).

Records in file order are i = 0 .. n-1; record i occupies [u[i], u[i+1]) of the inflated stream.  For a region (r, beg, end):
    R1          = records with ref == r, pos < beg and pos + covered > beg
    first_ge(x) = the first i with ref < 0, ref > r, or ref == r and pos >= x; else n
    a, b        = u[first_ge(beg)], u[first_ge(end)]
The output stream is the header bytes, then per region R1 and the bytes [a, b); every input block wholly inside [a, b) must be
in the output file byte for byte.  "*" alone: everything from the first record with ref < 0 on."""
import struct
import zlib

from tests.bamgen import CIGAR_OPS, EOF_BLOCK


def read_blocks(path):
    """[(file offset, file length, inflated bytes)] of the BGZF blocks in front of the first empty one."""
    data = open(path, "rb").read()
    out, o = [], 0
    while o < len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        isize = struct.unpack_from("<I", data, o + bsize - 4)[0]
        if isize == 0:
            break
        payload = zlib.decompress(data[o + 12 + xlen:o + bsize - 8], -15)
        assert len(payload) == isize
        out.append((o, bsize, payload))
        o += bsize
    return data, out


def inflate_file(path):
    """(inflated stream, [raw bytes of every block, the empty ones included])"""
    data = open(path, "rb").read()
    stream, raws, o = bytearray(), [], 0
    while o < len(data):
        xlen = struct.unpack_from("<H", data, o + 10)[0]
        bsize = struct.unpack_from("<H", data, o + 16)[0] + 1
        stream += zlib.decompress(data[o + 12 + xlen:o + bsize - 8], -15)
        raws.append(data[o:o + bsize])
        o += bsize
    return bytes(stream), raws


class Bam:
    def __init__(self, path):
        self.data, self.blocks = read_blocks(path)
        self.stream = b"".join(b[2] for b in self.blocks)
        self.block_start = [0]
        for b in self.blocks:
            self.block_start.append(self.block_start[-1] + len(b[2]))
        s = self.stream
        l_text = struct.unpack_from("<i", s, 4)[0]
        o = 8 + l_text
        n_ref = struct.unpack_from("<i", s, o)[0]
        o += 4
        self.refs = []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", s, o)[0]
            name = s[o + 4:o + 4 + l_name].rstrip(b"\0").decode()
            self.refs.append((name, struct.unpack_from("<i", s, o + 4 + l_name)[0]))
            o += 8 + l_name
        self.header_len = o
        self.recs = []          # (u, ref, pos, covered)
        while o < len(s):
            bs, ref, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiiBBHHH", s, o)
            cov = 0
            if not flag & 4:
                for k in range(n_cig):
                    c = struct.unpack_from("<I", s, o + 36 + l_name + 4 * k)[0]
                    if CIGAR_OPS[c & 15] in "MDN=X":
                        cov += c >> 4
            self.recs.append((o, ref, pos, cov))
            o += 4 + bs
        self.u = [r[0] for r in self.recs] + [len(s)]

    def first_ge(self, r, x):
        for i, (_, ref, pos, _) in enumerate(self.recs):
            if ref < 0 or ref > r or (ref == r and pos >= x):
                return i
        return len(self.recs)

    def region(self, text):
        if ":" in text:
            name, rng = text.rsplit(":", 1)
            beg, _, end = rng.partition("-")
            r = [n for n, _ in self.refs].index(name)
            return r, int(beg.replace(",", "")) - 1, int(end.replace(",", "")) if end else self.refs[r][1]
        r = [n for n, _ in self.refs].index(text)
        return r, 0, self.refs[r][1]

    def blocks_inside(self, a, b):
        return [self.data[o:o + n] for k, (o, n, _) in enumerate(self.blocks) if a <= self.block_start[k] and self.block_start[k + 1] <= b]


def slice_ref(path, regions):
    """regions: ["*"] or region strings / (ref id, beg, end) triples.  Returns (expected inflated stream, per region the raw input
    blocks that must appear verbatim, per region the records as bytes: R1 then [a, b) cut into records)."""
    bam = Bam(path)
    s = bam.stream
    out = bytearray(s[:bam.header_len])
    verbatim, records = [], []
    if list(regions) == ["*"]:
        i = next((k for k, r in enumerate(bam.recs) if r[1] < 0), len(bam.recs))
        out += s[bam.u[i]:]
        return bytes(out), [bam.blocks_inside(bam.u[i], len(s))], [[s[bam.u[k]:bam.u[k + 1]] for k in range(i, len(bam.recs))]]
    for g in regions:
        r, beg, end = bam.region(g) if isinstance(g, str) else g
        r1 = [k for k, (_, ref, pos, cov) in enumerate(bam.recs) if ref == r and pos < beg and pos + cov > beg]
        ia, ib = bam.first_ge(r, beg), bam.first_ge(r, end)
        a, b = bam.u[ia], bam.u[ib]
        for k in r1:
            out += s[bam.u[k]:bam.u[k + 1]]
        out += s[a:b]
        verbatim.append(bam.blocks_inside(a, b) if a < b else [])
        records.append([s[bam.u[k]:bam.u[k + 1]] for k in r1 + list(range(ia, ib))])
    return bytes(out), verbatim, records


def check_output(out_path, in_path, regions):
    """The four properties every case asserts; returns the number of verbatim blocks."""
    want, verbatim, _ = slice_ref(in_path, regions)
    got, raws = inflate_file(out_path)
    assert got == want, "inflated output differs from the definition (%d vs %d bytes)" % (len(got), len(want))
    assert raws and raws[-1] == EOF_BLOCK, "no EOF block at the end"
    flat = [b for v in verbatim for b in v]
    at = 0
    for b in flat:                                  # every listed block, byte for byte and in order
        while at < len(raws) - 1 and raws[at] != b:
            at += 1
        assert at < len(raws) - 1, "a block of the input that lies inside [a, b) was not copied verbatim"
        at += 1
    copied = set(flat)
    for b in raws[:-1]:                             # an empty block only where the input had it
        if struct.unpack_from("<I", b, len(b) - 4)[0] == 0:
            assert b in copied, "an empty block that is not a copied one"
    return len(flat)
