"""A DEFLATE (RFC 1951) writer for tests: streams are assembled bit by bit from explicit code lengths and explicit header operations,
so that a test can sit on the limits a decoder branches on -- code shapes, header encodings, token patterns -- which no encoder
emits on its own.  The writer tracks the payload it encodes; `sym`, `dsym` and `bits` emit anything at all, for invalid streams.
Plain Python, no dependencies.  Nothing here checks validity: that is zlib's job (tests/k1_cases.py)."""

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):                  # n bits of v, least significant first
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                  # a Huffman code: most significant bit first
        self.bits(int(format(c, "0%db" % n)[::-1], 2) if n else 0, n)

    def bitlen(self):
        return 8 * len(self.out) + self.n

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        assert self.n == 0
        return bytes(self.out)


def canonical_codes(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (RFC 1951 3.2.2); no validity check -- an over-subscribed
    set gets codes that overflow their length and are cut to it."""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


def kraft(lengths):
    """Sum of 2^(15 - l) over the codes: 32768 = complete, more = over-subscribed, less = incomplete."""
    return sum(1 << (15 - l) for l in lengths if l)


def complete_lengths(n):
    """Lengths of a complete code of n >= 2 symbols, as flat as possible (the shorter codes first)."""
    assert n >= 2
    k = n.bit_length() - 1
    r = n - (1 << k)
    return [k] * ((1 << k) - r) + [k + 1] * (2 * r)


def chain_lengths(first, last):
    """A complete code that reaches `last` bits and has nothing below `first`: 2^first - 1 codes of `first` bits, one each of
    first + 1 .. last - 1, two of `last` bits."""
    assert 1 <= first < last <= 15
    return [first] * ((1 << first) - 1) + list(range(first + 1, last)) + [last, last]


def lengths_of(symbols, lengths, n):
    """A list of n code lengths: symbols[i] gets lengths[i], every other symbol 0."""
    assert len(symbols) == len(lengths) and len(set(symbols)) == len(symbols)
    out = [0] * n
    for s, l in zip(symbols, lengths):
        out[s] = l
    return out


def default_ops(lens):
    """Header operations for a list of code lengths: ("L", v) a length, (16 | 17 | 18, count) a repeat -- greedy run lengths."""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                n = min(run, 138)
                ops.append((18, n))
                run -= n
            if run >= 3:
                ops.append((17, run))
                run = 0
            ops += [("L", 0)] * run
        else:
            ops.append(("L", v))
            run -= 1
            while run >= 3:
                n = min(run, 6)
                ops.append((16, n))
                run -= n
            ops += [("L", v)] * run
        i = j
    return ops


def expand_ops(ops):
    """The code lengths a list of header operations stands for (a 16 repeats the previous length, 0 after a 17 or 18)."""
    lens = []
    for op, x in ops:
        if op == "L":
            lens.append(x)
        elif op == 16:
            lens += [lens[-1] if lens else 0] * x
        else:
            lens += [0] * x
    return lens


def default_cl_lens(ops):
    """Code lengths of the code-length code for these operations: a complete code over the symbols in use (at least two), the
    frequent ones first."""
    freq = {}
    for op, x in ops:
        s = x if op == "L" else op
        freq[s] = freq.get(s, 0) + 1
    for s in (0, 8, 7):
        if len(freq) < 2:
            freq.setdefault(s, 0)
    order = sorted(freq, key=lambda s: (-freq[s], s))
    cl = [0] * 19
    for s, l in zip(order, complete_lengths(len(order))):
        cl[s] = l
    return cl


class Deflate:
    """A raw DEFLATE stream, block by block and token by token.  `payload` is what the tokens written so far inflate to."""

    def __init__(self):
        self.w, self.payload, self.lit_code, self.dist_code = BitWriter(), bytearray(), None, None

    # ---- blocks ----------------------------------------------------------------------------------------------------------
    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)
        return self

    def stored(self, data, final=False, length=None, nlen=None):
        data = bytes(data)
        length = len(data) if length is None else length
        self.header(final, 0)
        self.w.align()
        self.w.bits(length, 16)
        self.w.bits(length ^ 0xFFFF if nlen is None else nlen, 16)
        for b in data:
            self.w.bits(b, 8)
        self.payload += data
        return self

    def fixed(self, final=False):
        self.header(final, 1)
        self.lit_code, self.dist_code = canonical_codes(FIXED_LIT), canonical_codes(FIXED_DIST)
        return self

    def dynamic(self, lit_lens=None, dist_lens=None, final=False, ops=None, nlit=None, ndist=None, cl_lens=None, hclen=None):
        """A dynamic block header.  Either the code lengths (the operations are chosen by default_ops) or the operations and `nlit`
        (the lengths follow from them; what lies behind nlit is the distance code -- all of it, or `ndist` lengths where the operations
        run past the end on purpose; a leading 16 stands for zeros).  len(lit_lens) - 257 and
        len(dist_lens) - 1 go into the HLIT and HDIST fields as they are: 287 / 288 and 31 / 32 lengths write the invalid fields."""
        if ops is None:
            ops = default_ops(list(lit_lens) + list(dist_lens))
        else:
            lens = expand_ops(ops)
            lit_lens, dist_lens = lens[:nlit], lens[nlit:] if ndist is None else lens[nlit:nlit + ndist]
        if cl_lens is None:
            cl_lens = default_cl_lens(ops)
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]])
        assert 257 <= len(lit_lens) <= 288 and 1 <= len(dist_lens) <= 32 and 4 <= hclen <= 19
        assert all(cl_lens[s] == 0 for s in CL_ORDER[hclen:])
        self.header(final, 2)
        self.w.bits(len(lit_lens) - 257, 5)
        self.w.bits(len(dist_lens) - 1, 5)
        self.w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            self.w.bits(cl_lens[s], 3)
        cl = canonical_codes(cl_lens)
        for op, x in ops:
            if op == "L":
                self.w.code(*cl[x])
            else:
                self.w.code(*cl[op])
                lo, n = {16: (3, 2), 17: (3, 3), 18: (11, 7)}[op]
                self.w.bits(x - lo, n)
        self.lit_code, self.dist_code = canonical_codes(list(lit_lens)), canonical_codes(list(dist_lens))
        self.lit_lens, self.dist_lens = list(lit_lens), list(dist_lens)
        return self

    # ---- tokens ----------------------------------------------------------------------------------------------------------
    def sym(self, s):                      # any literal/length symbol that has a code
        self.w.code(*self.lit_code[s])
        return self

    def dsym(self, s):                     # any distance symbol that has a code
        self.w.code(*self.dist_code[s])
        return self

    def bits(self, v, n):
        self.w.bits(v, n)
        return self

    def lit(self, data):
        for b in bytes(data):
            self.sym(b)
            self.payload.append(b)
        return self

    def match(self, length, dist, lsym=None):
        """A match; lsym picks the length symbol where two can say it (284 with 31 extra = 285 = 258)."""
        if lsym is None:
            lsym = 285 if length == 258 else 257 + max(i for i in range(28) if LEN_BASE[i] <= length)
        li = lsym - 257
        self.sym(lsym)
        self.w.bits(length - LEN_BASE[li], LEN_EXTRA[li])
        di = max(i for i in range(30) if DIST_BASE[i] <= dist)
        self.dsym(di)
        self.w.bits(dist - DIST_BASE[di], DIST_EXTRA[di])
        self.copy(length, dist)
        return self

    def copy(self, length, dist):          # what a match does to the payload
        assert 1 <= dist <= len(self.payload)
        for _ in range(length):
            self.payload.append(self.payload[-dist])
        return self

    def eob(self):
        return self.sym(256)

    def finish(self):
        self.w.align()
        return self.w.bytes(), bytes(self.payload)
