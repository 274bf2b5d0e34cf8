"""K1b's write-out on the device: `lz77_resolve_body` (sambamba_amd/csrc/inflate.hip) stores a block's bytes as 16-byte groups at aligned
addresses and carries the < 16 bytes behind the last aligned address from batch to batch; single bytes are stored only in front of a
block's first aligned address and behind its last one, and neighbouring blocks share the group at their boundary.  Hand-assembled
blocks -- 1, 15, 16, 17, 31, 33 and 4097 bytes, one literal, an empty block between two others, one long run (a self-overlapping match:
batches cut at kSpanMax), 64 entries and then a last batch of 1, 5 or 15 bytes (fixed-code streams written token by token here), a
full 65280-byte block of BAM-like records -- are laid out back to back in groups that start at every residue mod 16, through the same
entry point as tests/test_gpu_inflate.py (sbx_inflate_blocks), and compared bit for bit with zlib.  The output buffer is filled with a
sentinel first: the entry point hands the bytes between and around the blocks through device memory, so a store outside a block's own
bytes shows.  (The plan itself runs on the CPU: tests/test_lz77_writeout_cpu.py.)"""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3
GAP = 80                     # sentinel bytes between two groups of blocks (a multiple of 16: the group's residue is set separately)

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
              16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class _FixedDeflate:
    """One final deflate block with the fixed code (RFC 1951, 3.2.6), written token by token."""

    def __init__(self):
        self.acc, self.n, self.out, self.payload = 0, 0, bytearray(), bytearray()
        self._bits(1, 1)
        self._bits(1, 2)

    def _bits(self, v, n):                 # n bits of v, least significant first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def _code(self, c, n):                 # a Huffman code: most significant bit first
        self._bits(int(format(c, "0%db" % n)[::-1], 2), n)

    def _sym(self, s):
        if s < 144:
            self._code(0x30 + s, 8)
        elif s < 256:
            self._code(0x190 + s - 144, 9)
        elif s < 280:
            self._code(s - 256, 7)
        else:
            self._code(0xC0 + s - 280, 8)

    def lit(self, data):
        for b in bytes(data):
            self._sym(b)
            self.payload.append(b)
        return self

    def match(self, length, dist):
        li = max(i for i in range(29) if _LEN_BASE[i] <= length) if length < 258 else 28
        self._sym(257 + li)
        self._bits(length - _LEN_BASE[li], _LEN_EXTRA[li])
        di = max(i for i in range(30) if _DIST_BASE[i] <= dist)
        self._code(di, 5)
        self._bits(dist - _DIST_BASE[di], _DIST_EXTRA[di])
        for _ in range(length):
            self.payload.append(self.payload[-dist])
        return self

    def finish(self):
        self._sym(256)
        if self.n:
            self._bits(0, 8 - self.n)
        return bytes(self.out), bytes(self.payload)


def _zlib_block(payload, level=6):
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    return co.compress(payload) + co.flush(), payload


def _entries_then_tail(rng, tail):
    """64 entries (a literal and a 3-byte match each: one full batch of K1b), then `tail` literals: a last batch of `tail` bytes."""
    d = _FixedDeflate()
    for k in range(64):
        d.lit(bytes([65 + k % 26])).match(3, 1)
    d.lit(rng.integers(0, 256, tail, dtype=np.uint8).tobytes())
    return d.finish()


def _records(rng, n, size):
    rec = bytearray(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
    out = bytearray()
    for _ in range(n):
        for _k in range(int(rng.integers(1, 6))):
            rec[int(rng.integers(0, size))] = int(rng.integers(0, 256))
        out += rec
    return bytes(out[:65280])


def _group(rng):
    """The blocks of one group, laid out back to back: (deflate stream, payload)."""
    rnd = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()     # noqa: E731
    blocks = [_FixedDeflate().lit(b"Q").finish()]                          # one literal
    blocks += [_zlib_block(rnd(n)) for n in (15, 16, 17)]
    blocks += [_zlib_block(b"")]                                           # an empty block between two others
    blocks += [_zlib_block(rnd(n)) for n in (31, 33, 1)]
    blocks += [_entries_then_tail(rng, t) for t in (1, 5, 15)]             # a last batch of < 16 bytes
    blocks += [_FixedDeflate().lit(b"R").match(258, 1).match(258, 1).match(200, 1).finish()]
    blocks += [_zlib_block(b"A" * 20011)]                                  # one long run: batches cut at kSpanMax
    blocks += [_zlib_block((rnd(97) * 50)[:4097])]
    blocks += [_zlib_block(_records(rng, 240, 283))]                       # a full block: the window slides, far and near matches
    return blocks


@pytest.fixture(scope="module")
def layout():
    rng = np.random.default_rng(20261)
    comp, co, cl, isz, oo, inside = bytearray(), [], [], [], [], []
    pos = 0

    def place(stream, payload):
        nonlocal pos
        assert zlib.decompress(stream, -15) == payload
        co.append(len(comp))
        cl.append(len(stream))
        isz.append(len(payload))
        oo.append(pos)
        inside.append((pos, payload))
        comp.extend(stream + b"\x5A\xA5\x5A")
        pos += len(payload)

    for r in range(16):
        pos += GAP
        pos += (r - pos) % 16                          # the group's first byte at residue r
        for stream, payload in _group(rng):
            place(stream, payload)
    # one byte behind a last gap, so that the bytes behind the last group are inside the buffer the entry point hands through
    pos += GAP
    place(*_FixedDeflate().lit(b"Z").finish())
    total = pos
    residues = {o % 16 for o in oo}
    assert residues == set(range(16))
    want = np.full(total, SENTINEL, np.uint8)
    for p, payload in inside:
        want[p:p + len(payload)] = np.frombuffer(payload, np.uint8)
    return np.frombuffer(bytes(comp), np.uint8), co, cl, isz, oo, want


def _inflate_into(comp, co, cl, isz, oo, out):
    import sambamba_amd
    from sambamba_amd._lib import lib
    a = [np.ascontiguousarray(comp, np.uint8), np.asarray(co, np.uint64), np.asarray(cl, np.uint32), np.asarray(isz, np.uint32), np.asarray(oo, np.uint64)]
    err = C.create_string_buffer(512)
    rc = lib().sbx_inflate_blocks(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(cl), out.ctypes.data,
                                  a[4].ctypes.data, err, 512)
    if rc != 0:
        raise sambamba_amd.SbxError(rc, err.value.decode())


def test_blocks_at_every_residue_bit_exact_and_nothing_around_them(layout):
    comp, co, cl, isz, oo, want = layout
    got = np.full(len(want), SENTINEL, np.uint8)
    _inflate_into(comp, co, cl, isz, oo, got)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing byte at %d (of %d), %d in all" % (bad[0], len(want), bad.size)
