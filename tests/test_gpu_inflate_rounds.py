"""K1b's phase B on the device, at its own decisions: the hand-assembled blocks of tests/lz77_round_cases.py -- (a) literals only: no near
match, no round; (b) 64 independent near matches in one batch: one round under the frontier test; (c) chains in which match i copies
match i - 1's output, 2, 3 and 63 deep: the exact rule, as many rounds; (d) (b) and (c) alternating batch by batch in one block; (e)
batches cut by the 1.5 KiB span at 2 and 63 entries and the 1-entry batch at a block's end (an entry is at most 513 bytes: the span
cannot cut below 2); (f) matches with dist 1, 8, 9 and 300 and len <= 16, 17 and 258 directly behind a one-round batch; and a random
token stream long enough for the window to slide -- go through the product path (sbx_inflate_blocks, as tests/test_gpu_inflate.py)
and are compared with zlib byte for byte.  The blocks lie back to back at odd addresses in a buffer filled with a sentinel, as in
tests/test_gpu_inflate_writeout.py, so a store outside a block's own bytes shows.  (The rounds' model on the CPU:
tests/test_lz77_rounds_cpu.py.)"""
import ctypes as C
import zlib

import numpy as np
import pytest

from tests.lz77_round_cases import cases

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3
GAP = 80


@pytest.fixture(scope="module")
def layout():
    comp, co, cl, isz, oo, inside, names = bytearray(), [], [], [], [], [], []
    pos = GAP + 5
    table = cases()
    # every block once behind a gap of sentinel bytes, then all of them again back to back (a block's neighbours are other blocks)
    for rep in range(2):
        for name, stream, payload, _, _, _, _ in table:
            assert zlib.decompress(stream, -15) == payload
            if rep == 0:
                pos += GAP + 3
            co.append(len(comp))
            cl.append(len(stream))
            isz.append(len(payload))
            oo.append(pos)
            inside.append((pos, payload))
            names.append(name)
            comp.extend(stream + b"\x5A\xA5\x5A")
            pos += len(payload)
    # one byte behind a last gap, so that the bytes behind the last block are inside the buffer the entry point hands through
    pos += GAP
    one = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = one.compress(b"Z") + one.flush()
    for lst, v in ((co, len(comp)), (cl, len(stream)), (isz, 1), (oo, pos), (inside, (pos, b"Z")), (names, "end")):
        lst.append(v)
    comp.extend(stream + b"\x5A\xA5\x5A")
    total = pos + 1
    want = np.full(total, SENTINEL, np.uint8)
    for p, payload in inside:
        want[p:p + len(payload)] = np.frombuffer(payload, np.uint8)
    return np.frombuffer(bytes(comp), np.uint8), co, cl, isz, oo, want, names


@pytest.fixture(scope="module")
def inflated(layout):
    import sambamba_amd
    from sambamba_amd._lib import lib
    comp, co, cl, isz, oo, want, _ = layout
    got = np.full(len(want), SENTINEL, np.uint8)
    a = [np.ascontiguousarray(comp, np.uint8), np.asarray(co, np.uint64), np.asarray(cl, np.uint32), np.asarray(isz, np.uint32), np.asarray(oo, np.uint64)]
    err = C.create_string_buffer(512)
    rc = lib().sbx_inflate_blocks(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(cl), got.ctypes.data,
                                  a[4].ctypes.data, err, 512)
    if rc != 0:
        raise sambamba_amd.SbxError(rc, err.value.decode())
    return got


@pytest.mark.parametrize("prefix", ["a_", "b_", "c_", "d_", "e_", "f_", "random_"])
def test_blocks_equal_zlib(layout, inflated, prefix):
    _, _, _, isz, oo, want, names = layout
    hit = 0
    for name, o, n in zip(names, oo, isz):
        if name.startswith(prefix):
            bad = np.flatnonzero(inflated[o:o + n] != want[o:o + n])
            assert bad.size == 0, "%s: first differing byte at %d of %d, %d in all" % (name, bad[0], n, bad.size)
            hit += 1
    assert hit >= 2


def test_nothing_around_the_blocks(layout, inflated):
    want = layout[5]
    bad = np.flatnonzero(inflated != want)
    assert bad.size == 0, "first differing byte at %d (of %d), %d in all" % (bad[0], len(want), bad.size)
