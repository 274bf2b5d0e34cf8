"""The case table of K1a (the Huffman decoders of inflate: the lane program sambamba_amd/csrc/inflate2_core.hpp and the general kernel
k_huffman_decode in inflate.hip), shared by tests/test_k1_cases_cpu.py and tests/test_gpu_k1_edges.py: hand-built DEFLATE streams
(tests/deflate_build.py) that sit on the limits the decoders branch on.  A case is (name, stream, payload or None, expect):

  payload  what the stream inflates to; None = the stream is invalid
  expect   Expect(path, loops, isize):
             path   "fast" the lane program decodes it, "general" it hands the block to the general kernel (stored blocks, more than
                    kMaxSeg = 6 deflate blocks, an incomplete literal/length code), "reject" both decoders refuse it
             loops  deflate blocks whose codes are not "plain" (a code of 1 or 2 bits, a literal/length code not complete within 14
                    bits, a distance code not complete within 12): a lane alone in its wavefront decodes them with the general form
                    of the symbol loop and every other block with the plain one
             isize  the ISIZE the block is given (the payload's length unless the defect is the ISIZE itself)

zlib is the reference of every expectation: the table is validated when it is built (a valid stream inflates to its payload within
ISIZE bytes and ends there; an invalid one is refused by zlib, or does not end at ISIZE) and no case is ever excluded.  The path of a
case is stated where it is built and checked against the rule above."""
import collections
import zlib

from tests.deflate_build import (DIST_BASE, DIST_EXTRA, LEN_BASE, LEN_EXTRA, Deflate, chain_lengths, complete_lengths, default_ops,
                                 kraft, lengths_of)

Expect = collections.namedtuple("Expect", "path loops isize")


def reference(stream, isize):
    """zlib's raw inflate of one BGZF block's payload into ISIZE bytes: the bytes, or an exception."""
    d = zlib.decompressobj(-15)
    out = d.decompress(stream, isize + 1)
    if not d.eof or len(out) != isize:
        raise ValueError("the stream does not end at ISIZE")
    return out


def _is_plain(lit_lens, dist_lens):
    short = any(l in (1, 2) for l in list(lit_lens) + list(dist_lens))
    return not short and kraft([l for l in lit_lens if l <= 14]) == 32768 and kraft([l for l in dist_lens if l <= 12]) == 32768


class Stream(Deflate):
    """A Deflate writer that keeps what the expectation is derived from."""

    def __init__(self):
        Deflate.__init__(self)
        self.n_huff = self.n_stored = self.n_fixed = self.loops = 0
        self.incomplete_lit = False

    def stored(self, *a, **kw):
        self.n_stored += 1
        return Deflate.stored(self, *a, **kw)

    def fixed(self, final=False):
        self.n_huff += 1
        self.n_fixed += 1
        return Deflate.fixed(self, final)

    def dynamic(self, *a, **kw):
        Deflate.dynamic(self, *a, **kw)
        self.n_huff += 1
        self.loops += 0 if _is_plain(self.lit_lens, self.dist_lens) else 1
        self.incomplete_lit = self.incomplete_lit or kraft(self.lit_lens) != 32768
        return self

    def code(self, lits, lsyms=(), dsyms=(), final=False, lit_shape=None, dist_shape=None, nlit=None, ndist=None, **kw):
        """A dynamic block over these literals, the end-of-block code, these length and distance symbols; the shapes default to flat
        complete codes, the symbols take the shape's lengths in the order given (literals, 256, length symbols)."""
        ls = sorted(set(bytes(lits))) + [256] + list(lsyms)
        lit_shape = complete_lengths(len(ls)) if lit_shape is None else lit_shape
        nlit = max(257, max(ls) + 1) if nlit is None else nlit
        ds = list(dsyms)
        if ds:
            dist_shape = (complete_lengths(len(ds)) if len(ds) > 1 else [1]) if dist_shape is None else dist_shape
            ndist = max(ds) + 1 if ndist is None else ndist
            dist_lens = lengths_of(ds, dist_shape, ndist)
        else:
            dist_lens = [0] * (1 if ndist is None else ndist)
        return self.dynamic(lengths_of(ls, lit_shape, nlit), dist_lens, final=final, **kw)


CASES = []
_names = set()
ALPHA = b"ACGTNacgtn=*"                      # 12 literals: with the end-of-block code and a length symbol or two a flat code of 4 bits


def _text(n, seed=1):
    out, x = bytearray(), seed
    for _ in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append(ALPHA[(x >> 16) % len(ALPHA)])
    return bytes(out)


def add(name, s, path, dyn_loops=None, isize=None, comp_len=None):
    """Registers a case.  `s` is a Stream (finished here) or raw bytes.  `dyn_loops` states how many of the case's DYNAMIC blocks have
    codes that are not plain (checked against the rule); Expect.loops is that number plus the case's fixed-code blocks, which are
    never plain -- the fixed code's 30 distance codes of 5 bits are not a complete code."""
    assert name not in _names, name
    _names.add(name)
    if isinstance(s, Stream):
        stream, payload = s.finish()
        derived = "general" if s.n_stored or s.n_huff > 6 or s.incomplete_lit else "fast"
        if path != "reject":
            assert path == derived, (name, path, derived)
            assert dyn_loops is None or dyn_loops == s.loops, (name, dyn_loops, s.loops)
            loops = s.loops + s.n_fixed
    else:
        stream, payload = bytes(s), None
    if comp_len is not None:
        stream = stream[:comp_len]
    isize = len(payload) if isize is None else isize
    assert isize <= 65536
    if path == "reject":
        try:
            reference(stream, isize)
        except (zlib.error, ValueError):
            pass
        else:
            raise AssertionError("zlib accepts the invalid case " + name)
        CASES.append((name, stream, None, Expect("reject", 0, isize)))
    else:
        assert reference(stream, isize) == payload, name
        CASES.append((name, stream, payload, Expect(path, loops, isize)))


def _history(s, n):
    """At least n bytes of output from a fixed-code block: a few literals and long matches."""
    s.fixed().lit(_text(40, 7))
    while len(s.payload) < n:
        s.match(258, 37)
    return s.eob()


# ---- code shapes ------------------------------------------------------------------------------------------------------------
def _code_shapes():
    # literal/length code that is complete only at 15 bits; a literal and a length symbol (284) hold the two 15-bit codes
    for last, loops in ((15, 1), (14, 0)):
        shape = chain_lengths(3, last)                        # 7 of 3 bits, 4 .. last - 1, two of `last` bits
        lits = bytes(range(65, 65 + len(shape) - 3)) + b"\xF0"
        s = Stream()
        # order: 256 and the first literals at 3 bits ... 0xF0 and 284 at the two longest codes
        ls = [256] + list(lits[:-1]) + [0xF0, 284]
        s.dynamic(lengths_of(ls, shape, 285), lengths_of(range(8), complete_lengths(8), 8), final=True)
        s.lit(lits).lit(b"\xF0\xF0").match(257, 3, lsym=284).lit(lits[::-1]).match(227, 1, lsym=284).lit(b"\xF0").match(250, 13, lsym=284)
        s.lit(b"\xF0" * 40).eob()
        add("lit_complete_only_at_15_bits" if last == 15 else "lit_complete_at_exactly_14_bits", s, "fast", loops)
    s = Stream()
    s.code(b"ABCD", [257], [0, 1], lit_shape=chain_lengths(1, 5), final=True)
    s.lit(b"AAAABACADAAAAAAAA").match(3, 1).lit(b"AAAA").match(3, 2).lit(b"DCBA" * 9).eob()
    add("lit_with_1_bit_symbol", s, "fast", 1)
    s = Stream()
    s.code(b"ABCDE", [257, 258], [0, 1, 2, 3, 4, 5, 6, 7], lit_shape=chain_lengths(2, 6), final=True)
    s.lit(b"ABCABCEEDDAA").match(4, 3).lit(b"BBB").match(3, 8).lit(b"EDCBA" * 7).eob()
    add("lit_with_2_bit_symbols", s, "fast", 1)
    # distance codes complete at exactly 12, 13 and 15 bits: the two longest codes and a short one in use
    for last, loops in ((12, 0), (13, 1), (15, 1)):
        shape = chain_lengths(3, last)
        nd = len(shape)
        s = Stream()
        s.code(ALPHA, [257, 258, 285], range(nd), dist_shape=shape)
        s.lit(_text(300, last))
        while len(s.payload) < DIST_BASE[nd - 1] + (1 << DIST_EXTRA[nd - 1]):
            s.match(258, 299)
        for ds in (nd - 1, nd - 2, 0, nd - 1, 7, nd - 2):
            s.lit(_text(2, ds)).match(4, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1).match(3, DIST_BASE[ds])
        s.lit(b"N").eob().fixed(True).lit(b"AC").match(5, 2).eob()
        add("dist_complete_at_exactly_%d_bits" % last, s, "fast", loops)
    s = Stream()
    s.code(ALPHA, [257, 258], range(5), dist_shape=chain_lengths(1, 4), final=True)
    s.lit(_text(20)).match(3, 1).match(4, 2).match(3, 3).match(3, 4).match(4, 5).match(3, 6).lit(b"A").match(3, 1).eob()
    add("dist_with_1_bit_symbols", s, "fast", 1)
    s = Stream()
    s.code(ALPHA, [257, 260], [0], final=True)
    s.lit(_text(9)).match(3, 1).lit(b"GT").match(6, 1).eob()
    add("dist_single_code_of_1_bit", s, "fast", 1)
    s = Stream()
    s.code(ALPHA, [], [], final=True).lit(_text(100)).eob()
    add("no_distance_code_hdist_0", s, "fast", 1)
    s = Stream()
    _history(s, 24577 + 8192)
    s.code(ALPHA, [257, 258], range(30), final=True)
    for ds in range(30):
        s.lit(_text(1, ds)).match(3 + ds % 2, DIST_BASE[ds] + (ds * 7) % (1 << DIST_EXTRA[ds]))
    s.eob()
    add("all_30_distance_symbols_used", s, "fast", 0)
    s = Stream()
    s.code(ALPHA, [], [], nlit=257, final=True).lit(_text(64, 3)).eob()
    add("hlit_257_no_length_symbols", s, "fast", 1)
    s = Stream()
    s.dynamic(complete_lengths(286), lengths_of(range(8), complete_lengths(8), 8), final=True)
    s.lit(bytes(range(256)))
    for ls in range(257, 286):
        s.match(LEN_BASE[ls - 257] + (1 << LEN_EXTRA[ls - 257]) - 1, 1 + ls % 6, lsym=ls).lit(bytes([ls & 0xFF]))
    s.lit(bytes(range(255, -1, -1))).eob()
    add("hlit_286_all_286_symbols_used", s, "fast", 0)
    s = Stream()
    s.dynamic(lengths_of([256], [1], 257), [0], final=True).eob()
    add("only_symbol_is_a_1_bit_end_of_block", s, "general")
    s = Stream()
    s.fixed().lit(b"before").eob().dynamic(lengths_of([256], [1], 257), [0]).eob().fixed(True).lit(b"after").match(4, 3).eob()
    add("1_bit_end_of_block_block_between_others", s, "general")


# ---- bit rate ---------------------------------------------------------------------------------------------------------------
def _bit_rate():
    # every iteration of the symbol loop at its most: a 15-bit literal, a 15-bit length symbol with 5 extra bits, a 15-bit distance
    # symbol with 13 extra bits (63 bits).  The shortest such match is 131 bytes and a block holds 65536: 24,6xx bytes of history
    # and then as many iterations as fit (about 300 back to back; 65536 bytes allow no more)
    s = Stream()
    _history(s, 24577 + 200)
    lshape, dshape = chain_lengths(1, 15), chain_lengths(1, 15)          # 1, 2, .. 14, 15, 15
    ls = [256] + list(range(66, 66 + 13)) + [0xF0, 281]
    s.dynamic(lengths_of(ls, lshape, 282), lengths_of(range(14, 30), dshape, 30), final=True)
    k = 0
    while len(s.payload) + 132 <= 65536:
        room = 65536 - len(s.payload) - 1
        length = min(131 + (k * 5 % 32 if k % 8 == 0 else 0), room)
        dist = min(24577 + (k * 977) % 8192, len(s.payload) + 1) if k % 2 else min(16385 + 8191 - k % 7, len(s.payload) + 1)
        s.lit(b"\xF0").match(length, dist, lsym=281)
        k += 1
    assert k >= 290
    s.lit(b"\xF0" * (65536 - len(s.payload))).eob()
    add("max_bit_rate_63_bits_per_iteration", s, "fast", 1)
    s = Stream()
    s.code(b"AB", lit_shape=[1, 2, 2], final=True).lit(b"A" * 60000).eob()
    add("one_bit_literals_60000", s, "fast", 1)


# ---- header encoding ----------------------------------------------------------------------------------------------------------
def _headers():
    # HCLEN = 4 leaves the code-length symbols 16, 17, 18 and 0 only: every code length is 0, there is no end-of-block code -- no
    # valid stream has it (an invalid case below).  The smallest HCLEN of a valid stream is 5 (symbol 8): 256 codes of 8 bits
    s = Stream()
    s.dynamic(ops=[("L", l) for l in [8] * 255 + [0, 8, 0]], nlit=257, final=True, cl_lens=lengths_of([0, 8], [1, 1], 19), hclen=5)
    s.lit(bytes(range(255)) * 2).eob()
    add("hclen_5_smallest_valid", s, "fast", 1)
    s = Stream()
    shape = chain_lengths(3, 15)
    ls = [256] + list(range(65, 65 + len(shape) - 3)) + [0xF0, 257]
    s.dynamic(lengths_of(ls, shape, 258), lengths_of(range(8), complete_lengths(8), 8), final=True, hclen=19)
    s.lit(b"ABCDEFGHIJ\xF0").match(3, 2).eob()
    add("hclen_19", s, "fast", 1)
    # all 19 code-length symbols in use, twelve of them with 7-bit codes: the sorted list crosses the 12 / 7 split
    s = Stream()
    lit = lengths_of([256] + list(range(40, 54)) + [257], chain_lengths(1, 15), 258)         # code lengths 1 .. 15 all occur
    dist = lengths_of(range(8), complete_lengths(8), 8)
    ops = default_ops(lit[:40]) + [("L", l) for l in lit[40:60]] + [(17, 5), ("L", 0), (18, 20), (17, 10), (18, 138), (17, 3), (17, 4), (18, 15)]
    assert len(ops) and sum(1 if o == "L" else x for o, x in ops) == 256
    ops += [("L", lit[256]), ("L", lit[257]), ("L", 3), (16, 6), ("L", 3)]
    cl = lengths_of([0, 18, 17, 16, 1, 2, 3] + [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15], [2, 2, 3, 3, 4, 4, 5] + [7] * 12, 19)
    s.dynamic(ops=ops, nlit=258, cl_lens=cl, final=True)
    assert s.lit_lens == lit and s.dist_lens == dist and {x if o == "L" else o for o, x in ops} == set(range(19))
    s.lit(bytes(range(40, 54))).match(3, 5).lit(b"(").eob()
    add("cl_all_19_symbols_7_bit_codes_across_12_7_split", s, "fast", 1)
    # repeats
    s = Stream()
    ops = [(18, 65), ("L", 4), (16, 6), (16, 4), (16, 3)] + [(18, 138), (18, 256 - 65 - 14 - 138)] + [("L", 4), ("L", 4)] + [("L", 3), (16, 3), (16, 4)]
    s.dynamic(ops=ops, nlit=258, final=True)              # 'A' .. 'N', 256 and 257 at 4 bits; 8 distance symbols of 3
    s.lit(b"ABCDEFGHIJKLMN").match(3, 8).lit(b"NMLK").match(3, 1).eob()
    add("rep16_in_a_chain_and_rep18_of_138", s, "fast", 0)
    s = Stream()
    # a 16 directly behind a 17 and behind an 18 repeats 0
    ops = [(17, 3), (16, 3), (18, 50), (16, 6), (17, 3)] + [("L", 4)] * 14 + [(18, 138), (16, 5), (18, 256 - 79 - 143)] + [("L", 4), ("L", 4)]
    ops += [("L", 3)] * 8
    s.dynamic(ops=ops, nlit=258, final=True)
    assert s.lit_lens[:65] == [0] * 65 and s.lit_lens[65] == 4
    s.lit(b"ABCDEFGHIJKLMN").match(3, 14).eob()
    add("rep16_directly_after_17_and_after_18", s, "fast", 0)
    s = Stream()
    # a 16 that starts in the literal/length lengths and ends in the distance lengths (nlit = 260: four of its six lengths are distance lengths)
    lit = lengths_of(list(ALPHA) + [256, 257, 258, 259], [4] * 16, 260)
    ops = default_ops(lit[:257]) + [("L", 4), (16, 6)] + [("L", 3)] * 6
    s.dynamic(ops=ops, nlit=260, final=True)
    assert s.lit_lens == lit and s.dist_lens == [4] * 4 + [3] * 6 and kraft(s.dist_lens) == 32768
    s.lit(_text(40)).match(5, 32).match(5, 1).match(3, 17).eob()
    add("rep16_across_the_hlit_boundary", s, "fast", 0)
    s = Stream()
    # an 18 across the boundary: the zeros of 258 .. 285 and of the first 12 distance symbols (138 zeros cannot cross it in a
    # valid stream: 29 lengths behind the end-of-block code and 30 distance lengths at the most)
    ops = default_ops(lengths_of(list(ALPHA) + [256, 257], complete_lengths(14), 258)) + [(18, 28 + 12)] + [("L", 1), ("L", 1)]
    s.dynamic(ops=ops, nlit=286, final=True)
    assert len(s.dist_lens) == 14
    s.lit(_text(200)).match(3, 65).match(3, 97).match(3, 128).match(3, 96).eob()
    add("rep18_across_the_hlit_boundary", s, "fast", 1)
    s = Stream()
    lit = lengths_of(list(ALPHA) + [256, 257, 258, 259], [4] * 16, 260)
    ops = default_ops(lit) + [("L", 1), ("L", 1), (18, 28)]
    s.dynamic(ops=ops, nlit=260, final=True)
    assert len(s.dist_lens) == 30
    s.lit(_text(30)).match(3, 1).match(5, 2).eob()
    add("rep18_ends_exactly_at_nlit_plus_ndist", s, "fast", 1)
    s = Stream()
    ops = default_ops(lit) + [("L", 3), (16, 6), ("L", 3)]
    s.dynamic(ops=ops, nlit=260, final=True)
    s.lit(_text(30)).match(3, 5).match(5, 13).eob()
    add("rep16_then_length_ends_exactly_at_nlit_plus_ndist", s, "fast", 0)
    s = Stream()
    ops = default_ops(lit) + [("L", 3), ("L", 3), (16, 6)]
    s.dynamic(ops=ops, nlit=260, final=True)
    s.lit(_text(30)).match(3, 5).match(5, 13).eob()
    add("rep16_ends_exactly_at_nlit_plus_ndist", s, "fast", 0)
    # nlit at every position of the dword of eight code lengths the distance lengths begin in
    for nlit in (257, 258, 263, 264, 265, 286):
        s = Stream()
        lsyms = list(range(257, nlit))[-3:]
        n = 12 + 1 + len(lsyms)
        shape = complete_lengths(n)
        s.code(ALPHA, lsyms, range(9), nlit=nlit, lit_shape=shape, final=True)
        s.lit(_text(40, nlit))
        for k, ls in enumerate(lsyms):
            s.match(LEN_BASE[ls - 257], 1 + 5 * k, lsym=ls).lit(_text(3, k))
        if nlit == 257:
            s.lit(_text(17, 5))
        else:
            s.match(LEN_BASE[lsyms[0] - 257], 24, lsym=lsyms[0]).match(LEN_BASE[lsyms[-1] - 257], 9, lsym=lsyms[-1])
        s.eob()
        add("nlit_%d" % nlit, s, "fast", 0)


# ---- tokens -------------------------------------------------------------------------------------------------------------------
def _tokens():
    for n in (254, 255, 256, 509, 510, 511):
        s = Stream()
        s.code(ALPHA, [257, 258], range(8), final=True).lit(_text(n, n)).match(4, 1 + n % 16).lit(b"A").eob()
        add("lits_%d_then_match" % n, s, "fast", 0)
        s = Stream()
        s.code(ALPHA, [257, 258], range(8)).lit(_text(n, n)).eob().fixed(True).match(3, 2).lit(b"xy").eob()
        add("lits_%d_then_end_of_block" % n, s, "fast", 0)
        s = Stream()
        s.fixed().lit(b"Q").match(5, 1).eob().code(ALPHA, [257, 258], range(8), final=True).lit(_text(n, n)).eob()
        add("lits_%d_at_end_of_stream" % n, s, "fast", 0)
    # a literal run over two deflate blocks with different codes (two translation tables), split inside the second; then a match
    s = Stream()
    s.code(b"abcdefghijkl", [257], range(8)).lit(b"abcdefghijkl" * 16 + b"lkj").eob()               # 195 literals
    s.code(b"lkjihgfedcbaZYXW", [258, 259], range(18), final=True).lit(b"ZalYbkXcjW" * 10).match(4, 290).lit(b"Z").match(5, 1).eob()
    add("lit_run_over_two_blocks_with_different_codes_then_match", s, "fast", 0)
    s = Stream()
    s.code(b"abcdefghijkl", [257], range(8)).lit(b"abcdefghijkl" * 21).eob()                            # 252
    s.code(b"lkjihgfedcbaZYXW", [258, 259], range(18), final=True).lit(b"ZaY").match(4, 255).eob()       # 255: the split and the match meet
    add("lit_run_of_255_over_two_blocks_then_match", s, "fast", 0)
    s = Stream()
    s.code(ALPHA, [257, 258], range(8), final=True).lit(_text(65536, 11)).eob()
    add("lits_65536_no_match_isize_65536", s, "fast", 0)
    # every length symbol at its least and most extra bits, 284 with 31 extra bits (258, as zlib reads it) and 285
    s = Stream()
    s.fixed(True).lit(b"lengths")
    for ls in range(257, 286):
        i = ls - 257
        s.match(LEN_BASE[i], 1 + i % 7, lsym=ls).lit(b"-").match(LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1, 2 + i % 5, lsym=ls)
    s.eob()
    assert LEN_BASE[27] + 31 == 258
    add("every_length_symbol_least_and_most_extra_bits", s, "fast", 0)
    s = Stream()
    _history(s, 32768)
    s.fixed(True)
    for ds in range(30):
        s.match(3, DIST_BASE[ds]).lit(b"d").match(4, DIST_BASE[ds] + (1 << DIST_EXTRA[ds]) - 1)
    s.eob()
    add("every_distance_symbol_least_and_most_extra_bits", s, "fast", 0)
    s = Stream()
    s.fixed(True).lit(b"a").match(3, 1).lit(b"bc").match(6, 6).lit(_text(300)).match(258, 312).match(3, 570).eob()
    add("distance_equal_to_the_bytes_produced", s, "fast", 0)
    s = Stream()
    s.fixed().lit(_text(32768, 5)).eob().fixed(True).match(258, 32768).match(258, 32768).lit(b"A").match(3, 32768).eob()
    add("distance_32768", s, "fast", 0)
    s = Stream()
    s.fixed(True).lit(b"Z").match(258, 1).lit(b"Y").match(258, 1).eob()
    add("distance_1_length_258", s, "fast", 0)
    s = Stream()
    s.fixed(True).lit(_text(50)).match(258, 50).eob()
    add("match_ends_exactly_at_isize", s, "fast", 0)
    s = Stream()
    s.fixed(True).lit(_text(190))
    while len(s.payload) + 258 <= 65536:
        s.match(258, 190)
    s.match(65536 - len(s.payload), 77).eob()
    assert len(s.payload) == 65536
    add("match_ends_exactly_at_isize_65536", s, "fast", 0)
    # the most entries a block can have: 3-byte matches throughout
    s = Stream()
    s.code(b"AB", [257, 258, 259, 260, 261], range(8), final=True).lit(b"A")
    for k in range(21845):
        s.match(3, 1 + k % 3 if k > 2 else 1)
    s.eob()
    assert len(s.payload) == 65536
    add("most_entries_3_byte_matches_throughout", s, "fast", 0)
    s = Stream()
    s.code(ALPHA, [257, 258], range(8), final=True)
    while len(s.payload) + 255 + 3 * 400 <= 65536:
        s.lit(_text(255, len(s.payload)))
        for k in range(400):
            s.match(3, 1 + k % 16)
    s.lit(_text(65536 - len(s.payload), 2)).eob()
    add("most_entries_3_byte_matches_and_255_literal_splits", s, "fast", 0)


# ---- deflate blocks per BGZF block ------------------------------------------------------------------------------------------------
def _blocks():
    for n in (1, 5, 6, 7, 40):
        s = Stream()
        for k in range(n):
            final = k == n - 1
            if k % 2:
                s.fixed(final).lit(_text(20 + k, k)).match(3 + k % 5, 7).eob()
            else:
                s.code(ALPHA[k % 3:], [257, 258, 259, 260, 261], range(8), final=final).lit(_text(30, k).translate(None, ALPHA[:k % 3]) + b"Tn")
                s.match(5, 1).eob()
        add("deflate_blocks_%d" % n, s, "fast" if n <= 6 else "general", 0)
    s = Stream()
    s.fixed(True).eob()
    add("empty_block", s, "fast", 0)
    s = Stream()
    s.fixed(True).lit(b"1").eob()
    add("one_byte_block", s, "fast", 0)
    s = Stream()
    s.fixed().lit(b"one").eob().fixed().eob().code(ALPHA, [257], range(8)).eob().fixed().lit(b"two").match(3, 3).eob()
    s.code(ALPHA, [257, 258, 259], range(8)).eob().fixed(True).eob()
    add("empty_fixed_and_dynamic_blocks_between_others", s, "fast", 0)
    s = Stream()
    s.fixed().lit(_text(30)).match(9, 30).eob().code(ALPHA, [257, 258, 259], range(12)).lit(_text(30, 2)).match(3, 60).eob()
    s.fixed(True).match(11, 41).lit(b"end").eob()
    add("fixed_dynamic_fixed", s, "fast", 0)


# ---- stored blocks: the general kernel's ---------------------------------------------------------------------------------------------
def _stored():
    s = Stream()
    s.stored(b"").fixed(True).lit(b"abc").match(3, 3).eob()
    add("stored_len_0_at_the_start", s, "general")
    s = Stream()
    s.fixed().lit(b"abc").eob().stored(b"").fixed(True).match(3, 3).eob()
    add("stored_len_0_in_the_middle", s, "general")
    s = Stream()
    s.fixed().lit(b"abc").match(3, 3).eob().stored(b"", final=True)
    add("stored_len_0_as_the_final_block", s, "general")
    seen = set()
    for k in range(8):
        s = Stream()
        s.fixed().lit(b"\xF0" * k + b"AB").match(3, 1).eob()          # 9-bit literals: k more bits
        off = s.w.bitlen() % 8
        seen.add(off)
        s.stored(_text(21, k)).fixed(True).match(4, 20).eob()
        add("stored_after_huffman_data_ending_at_bit_%d" % off, s, "general")
    assert seen == set(range(8))
    s = Stream()
    s.stored(_text(65535, 9)).fixed(True).lit(b"!").eob()
    add("stored_65535_bytes_plus_one_literal", s, "general")
    s = Stream()
    s.fixed().lit(b"head").eob().stored(_text(300, 4)).fixed(True).match(258, 300).match(3, 304).match(10, 1).eob()
    add("matches_that_reach_back_into_stored_bytes", s, "general")


# ---- placement: payloads of 1 .. 70 bytes (the tests lay them out at every address mod 16) --------------------------------------------
PLACEMENT = ["placement_%d_bytes" % n for n in range(1, 71)]


def _placement():
    for n in range(1, 71):
        s = Stream()
        if n % 3 == 0:
            s.code(ALPHA, [257, 258, 259], range(8), final=True)
        else:
            s.fixed(True)
        k = min(n, 1 + n % 5)
        s.lit(_text(k, n))
        while len(s.payload) < n:
            m = n - len(s.payload)
            if m >= 3:
                s.match(min(m, 5), 1 + n % k)
            else:
                s.lit(_text(m, n + 1))
        s.eob()
        add("placement_%d_bytes" % n, s, "fast", 0)


# ---- invalid streams: the named defect is the only thing wrong ------------------------------------------------------------------------
def _invalid():
    flat16 = lengths_of(list(ALPHA) + [256, 257, 258, 259], [4] * 16, 260)
    d8 = [3] * 8

    def ops18(lens):                       # lengths one by one, zeros in runs of 18: the code-length symbols 0, 3, 4 and 18 alone
        ops, i = [], 0
        while i < len(lens):
            run = 0
            while i + run < len(lens) and lens[i + run] == 0 and run < 138:
                run += 1
            ops += [(18, run)] if run >= 11 else [("L", l) for l in lens[i:i + max(run, 1)]]
            i += max(run, 1)
        return ops

    def ok_tail(s):
        return s.lit(_text(20)).match(4, 5).eob()

    s = Stream()
    s.fixed().lit(b"abc").eob().header(True, 3)
    add("bad_btype_3", s, "reject")
    s = Stream()
    s.fixed().lit(b"abc").eob().stored(b"defg", final=True, nlen=0xFFFB ^ 1)
    add("bad_stored_nlen_mismatch", s, "reject")
    s = Stream()
    s.fixed().lit(b"abc").eob().stored(b"0123456789", final=True)
    add("bad_stored_len_beyond_isize", s, "reject", isize=12)
    for field in (30, 31):
        s = Stream()
        ok_tail(s.dynamic(flat16 + [0] * (257 + field - 260), d8, final=True))
        add("bad_hlit_field_%d" % field, s, "reject")
        s = Stream()
        ok_tail(s.dynamic(flat16, d8 + [0] * (field + 1 - 8), final=True))
        add("bad_hdist_field_%d" % field, s, "reject")
    s = Stream()
    ok_tail(s.dynamic(ops=ops18(flat16 + d8), nlit=260, final=True, cl_lens=lengths_of([0, 3, 4, 18], [1, 2, 2, 2], 19)))
    add("bad_code_length_code_oversubscribed", s, "reject")
    s = Stream()
    ok_tail(s.dynamic(ops=ops18(flat16 + d8), nlit=260, final=True, cl_lens=lengths_of([0, 3, 4, 18], [1, 2, 3, 4], 19)))       # the code 1111 is missing and never used
    add("bad_code_length_code_incomplete_missing_code_unused", s, "reject")
    s = Stream()
    s.dynamic(ops=[("L", l) for l in [8] * 255 + [0, 8, 0]], nlit=257, final=True, cl_lens=lengths_of([0, 8], [1, 2], 19))   # two codes, 0 and 10
    s.lit(b"abc").eob()
    add("bad_code_length_code_of_two_codes_incomplete", s, "reject")
    s = Stream()
    # a decoder without the check takes the leading 16 for three zeros -- the lengths of the symbols 0 .. 2, which are zeros -- and finds
    # complete codes, tokens, an end-of-block code and ISIZE bytes behind it
    assert flat16[:3] == [0, 0, 0]
    ok_tail(s.dynamic(ops=[(16, 3)] + default_ops(flat16[3:] + d8), nlit=260, final=True))
    assert s.lit_lens == flat16 and s.dist_lens == d8
    add("bad_first_operation_is_a_16", s, "reject")
    s = Stream()
    # HDIST says 10 distance lengths; the last operation, a 17 of 3, writes the two zeros that are left and one more.  A decoder
    # without the check has the codes of the first nlit + ndist lengths and finds tokens, an end-of-block code and ISIZE bytes
    ok_tail(s.dynamic(ops=default_ops(flat16 + d8) + [(17, 3)], nlit=260, ndist=10, final=True))
    assert s.lit_lens == flat16 and s.dist_lens == d8 + [0, 0]
    add("bad_repeat_past_nlit_plus_ndist", s, "reject")
    s = Stream()
    s.dynamic(lengths_of(list(ALPHA) + [255, 257, 258, 259], [4] * 16, 260), d8, final=True).lit(_text(20)).match(4, 5).sym(255)
    add("bad_no_end_of_block_code", s, "reject", isize=24)
    s = Stream()
    ok_tail(s.dynamic(lengths_of(list(ALPHA) + [256, 257, 258, 259, 260], [4] * 15 + [3, 3], 261), d8, final=True))
    add("bad_literal_length_code_oversubscribed", s, "reject")
    s = Stream()
    ok_tail(s.dynamic(lengths_of(list(ALPHA) + [256, 257, 258], [4] * 15, 259), d8, final=True))             # 15 of the 16 codes of 4 bits
    add("bad_literal_length_code_incomplete_missing_code_unused", s, "reject")
    s = Stream()
    s.dynamic(lengths_of([65, 256], [2, 2], 257), [0], final=True).lit(b"AAAA").eob()
    add("bad_literal_length_code_of_two_2_bit_codes", s, "reject")
    s = Stream()
    ok_tail(s.dynamic(flat16, [2] * 3 + [3] * 3, final=True))
    add("bad_distance_code_oversubscribed", s, "reject")
    s = Stream()
    s.dynamic(flat16, [2, 2], final=True).lit(_text(20)).match(4, 1).match(3, 2).eob()
    add("bad_distance_code_incomplete_two_2_bit_codes", s, "reject")
    s = Stream()
    s.dynamic(flat16, [0, 0, 0, 0, 3], final=True).lit(_text(20)).match(4, 5).eob()                           # one code, but not of 1 bit
    add("bad_distance_code_single_code_of_3_bits", s, "reject")
    s = Stream()
    s.dynamic(flat16, [1], final=True).lit(_text(20)).match(4, 1).sym(257).bits(1, 1).lit(b"A").eob()         # the code `1` has no symbol
    add("bad_unused_code_of_the_single_code_distance_tree", s, "reject", isize=20 + 4 + 3 + 1)
    for bad in (286, 287):
        s = Stream()
        s.fixed(True).lit(b"abcd").sym(bad).bits(0, 5).lit(b"e").eob()
        add("bad_fixed_code_symbol_%d" % bad, s, "reject", isize=4 + 3 + 1)
    for bad in (30, 31):
        s = Stream()
        s.fixed(True).lit(b"abcd").sym(257).dsym(bad).lit(b"e").eob()
        add("bad_fixed_distance_code_%d" % bad, s, "reject", isize=4 + 3 + 1)
    s = Stream()
    s.fixed(True).lit(b"abc").sym(257).dsym(3).lit(b"e").eob()           # distance 4 behind 3 bytes
    add("bad_distance_one_more_than_the_bytes_produced", s, "reject", isize=3 + 3 + 1)
    s = Stream()
    s.fixed(True).lit(_text(300)).sym(258).dsym(16).bits(301 - 257, 7).eob()        # distance 301 behind 300 bytes, behind a split run
    add("bad_distance_301_behind_300_literals", s, "reject", isize=300 + 4)
    s = Stream()
    s.fixed(True).lit(_text(50)).match(10, 50).eob()
    add("bad_match_one_byte_past_isize", s, "reject", isize=59)
    s = Stream()
    s.fixed(True).lit(_text(50)).match(10, 50).lit(b"A").eob()
    add("bad_literal_one_byte_past_isize", s, "reject", isize=60)
    s = Stream()
    s.fixed(True).lit(_text(50)).match(10, 50).eob()
    add("bad_final_end_of_block_before_isize", s, "reject", isize=61)
    s = Stream()
    s.code(ALPHA, [257, 258], range(8), final=True).lit(_text(200)).match(4, 9).lit(_text(200, 2)).eob()
    add("bad_comp_len_cut_in_the_middle_of_a_symbol", s, "reject", comp_len=90)
    s = Stream()
    s.fixed().lit(_text(50)).match(10, 50).eob()
    add("bad_no_final_block", s, "reject")
    s = Stream()
    s.dynamic(ops=[(18, 138), (18, 120), (17, 3)], nlit=260, final=True, cl_lens=lengths_of([18, 17], [1, 1], 19), hclen=4)
    add("bad_hclen_4_every_code_length_0", s.finish()[0], "reject", isize=0)


for _f in (_code_shapes, _bit_rate, _headers, _tokens, _blocks, _stored, _placement, _invalid):
    _f()

VALID = [c for c in CASES if c[2] is not None]
INVALID = [c for c in CASES if c[2] is None]
BY_NAME = {c[0]: c for c in CASES}


def case_file(cases, path):
    """The cases as the file tests/cpp/inflate2_host.cpp reads in its --cases mode: per case u32 name length, name, u32 expectation
    (0 fast, 1 general, 2 reject), u32 loops, u32 ISIZE, u32 stream length, stream, payload (ISIZE bytes; none for a reject)."""
    import struct
    with open(path, "wb") as fh:
        for name, stream, payload, e in cases:
            nm = name.encode()
            fh.write(struct.pack("<I", len(nm)) + nm)
            fh.write(struct.pack("<IIII", ("fast", "general", "reject").index(e.path), e.loops or 0, e.isize, len(stream)))
            fh.write(stream)
            if payload is not None:
                fh.write(payload)
