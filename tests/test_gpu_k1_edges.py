"""K1a on the device over the case table (tests/k1_cases.py): hand-built DEFLATE streams at the limits the two Huffman decoders branch
on -- k_huffman_decode2 (the lane program inflate2_core.hpp) and the general kernel k_huffman_decode (sambamba_amd/csrc/inflate.hip).
zlib is the reference (the table is validated against it when it is built); every stream has passed the lane program on the CPU, under
AddressSanitizer with exactly the documented readable bytes behind it (tests/test_k1_cases_cpu.py), before it comes here.  Everything
goes through sbx_inflate_blocks with a sentinel-filled output: the bytes between the blocks make the round trip through device memory,
so a store outside a block's own bytes shows.  Block b of a call is lane b % 64 of wavefront b // 64."""
import ctypes as C

import numpy as np
import pytest

from tests import k1_cases

pytestmark = pytest.mark.gpu

SENTINEL = 0xC3
JUNK = b"\x5A\xA5\x5A"


def _call(blocks, residues=None, tight_end=False):
    """One sbx_inflate_blocks call over (stream, isize, payload) blocks.  The streams lie back to back with three junk bytes between
    them, or at the address mod 16 that `residues` names; the outputs lie 17 .. 48 sentinel bytes apart.  Returns (got, want)."""
    import sambamba_amd
    from sambamba_amd._lib import lib
    comp, co, cl, isz, oo, inside = bytearray(), [], [], [], [], []
    pos = 0
    for k, (stream, isize, payload) in enumerate(blocks):
        if residues is not None:
            comp.extend(b"\xA5" * ((residues[k] - len(comp)) % 16))
        pos += 17 + (k * 7) % 32
        co.append(len(comp))
        cl.append(len(stream))
        isz.append(isize)
        oo.append(pos)
        inside.append((pos, payload))
        comp.extend(stream)
        if not (tight_end and k == len(blocks) - 1):
            comp.extend(JUNK if payload is not None else bytes(8))     # (behind an invalid stream: zeros, a stored header that is refused)
        pos += isize
    pos += 40
    want = np.full(pos, SENTINEL, np.uint8)
    for p, payload in inside:
        if payload is not None:
            want[p:p + len(payload)] = np.frombuffer(payload, np.uint8)
    got = np.full(pos, SENTINEL, np.uint8)
    a = [np.frombuffer(bytes(comp), np.uint8), np.asarray(co, np.uint64), np.asarray(cl, np.uint32), np.asarray(isz, np.uint32), np.asarray(oo, np.uint64)]
    err = C.create_string_buffer(512)
    rc = lib().sbx_inflate_blocks(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, len(cl), got.ctypes.data,
                                  a[4].ctypes.data, err, 512)
    if rc != 0:
        raise sambamba_amd.SbxError(rc, err.value.decode())
    return got, want


def _same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first differing byte at %d (of %d), %d in all" % (bad[0], len(want), bad.size)


def _block(name):
    _, stream, payload, e = k1_cases.BY_NAME[name]
    return stream, e.isize, payload


PLAIN = [c[0] for c in k1_cases.VALID if c[3].path == "fast" and c[3].loops == 0 and c[3].isize <= 4096]
KEPT = [c[0] for c in k1_cases.VALID if c[3].path == "fast" and c[3].isize <= 4096]


def test_plain_blocks_exist():
    assert len(PLAIN) >= 30 and "nlit_264" in PLAIN and "lit_complete_at_exactly_14_bits" in PLAIN
    assert k1_cases.BY_NAME["lit_complete_only_at_15_bits"][3].loops == 1


def test_every_valid_case_in_one_call_bit_exact_and_nothing_around_it():
    blocks = [(stream, e.isize, payload) for _, stream, payload, e in k1_cases.VALID]
    _same(*_call(blocks))


def test_payloads_of_1_to_70_bytes_at_every_address_mod_16():
    """... of the compressed buffer; the last one ends the buffer: nothing of the caller's lies behind its last byte."""
    blocks, residues = [], []
    for r in range(16):
        for name in k1_cases.PLACEMENT:
            blocks.append(_block(name))
            residues.append((r + len(blocks)) % 16)
    seen = {(i % 70, residues[i]) for i in range(len(blocks))}
    assert len(seen) == 70 * 16
    _same(*_call(blocks, residues=residues, tight_end=True))


def _wave(n, fill, special):
    """n blocks: `fill` names in turn, `special` {block index: name}."""
    return [_block(special.get(b, fill[b % len(fill)])) for b in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_wavefronts_of_plain_blocks_only(n):
    _same(*_call(_wave(n, PLAIN, {})))


@pytest.mark.parametrize("n,at", [(64, 0), (64, 31), (64, 63), (65, 64), (129, 127), (129, 128)])
@pytest.mark.parametrize("name", ["lit_complete_only_at_15_bits", "dist_complete_at_exactly_13_bits", "lit_with_1_bit_symbol"])
def test_one_block_forces_the_other_63_off_the_plain_loop(n, at, name):
    _same(*_call(_wave(n, PLAIN, {at: name})))


@pytest.mark.parametrize("n,at", [(64, 0), (64, 40), (65, 63), (129, 64), (129, 128)])
@pytest.mark.parametrize("name", ["deflate_blocks_7", "stored_after_huffman_data_ending_at_bit_5", "only_symbol_is_a_1_bit_end_of_block"])
def test_one_block_handed_to_the_general_kernel_among_those_the_fast_one_keeps(n, at, name):
    _same(*_call(_wave(n, KEPT, {at: name})))


@pytest.mark.parametrize("n,at", [(64, 0), (64, 63), (129, 100)])
@pytest.mark.parametrize("name", ["lits_65536_no_match_isize_65536", "match_ends_exactly_at_isize_65536", "most_entries_3_byte_matches_throughout",
                                  "most_entries_3_byte_matches_and_255_literal_splits"])
def test_one_65536_byte_block_among_empty_and_one_byte_blocks(n, at, name):
    got, want = _call(_wave(n, ["empty_block", "one_byte_block"], {at: name}))
    _same(got, want)


@pytest.mark.parametrize("n,a,b", [(64, 0, 1), (64, 5, 63), (129, 64, 127), (129, 128, 3)])
def test_the_fastest_and_the_slowest_consumer_of_input_share_a_wavefront(n, a, b):
    """63 bits per iteration beside 2 bits per iteration: the input ring of the one is served at the pace the other asks for."""
    _same(*_call(_wave(n, PLAIN, {a: "max_bit_rate_63_bits_per_iteration", b: "one_bit_literals_60000"})))


@pytest.mark.parametrize("name", [c[0] for c in k1_cases.INVALID])
def test_invalid_stream_is_refused(name):
    """Between two valid blocks; input validation of a stream the CPU run has shown to stay inside its bounds."""
    import sambamba_amd
    with pytest.raises(sambamba_amd.SbxError) as ei:
        _call([_block("nlit_264"), _block(name), _block("fixed_dynamic_fixed")])
    assert ei.value.code == -3 and ei.value.msg.startswith("block 1:")
