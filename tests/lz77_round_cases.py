"""Hand-assembled deflate blocks that sit on the decisions of K1b's phase B (sambamba_amd/csrc/inflate.hip, lz77_resolve_body): whether
a batch has a near match at all, whether one round under the frontier test finishes it (lz::frontier_blocked, the one-round fast path),
how deep its dependency chain is, where the 1.5 KiB span cuts it, and which copy path a match takes.  Written token by token with
tests/deflate_build.py (fixed code), so that the entries K1a hands to K1b are known: a batch is the next 64 entries, or fewer where
their output would pass 1536 bytes.  Shared by tests/test_lz77_rounds_cpu.py (the lock-step model) and tests/test_gpu_inflate_rounds.py."""
import random

from tests.deflate_build import Deflate

SPAN_MAX = 1536


class Tokens:
    """A fixed-code deflate block, and next to it the entries and literals as K1a emits them."""

    def __init__(self, seed):
        self.d = Deflate().fixed(final=True)
        self.rng = random.Random(seed)
        self.entries, self.literals, self.run = [], bytearray(), 0

    @property
    def pos(self):
        return len(self.d.payload)

    def lit(self, n):
        data = bytes(self.rng.randrange(256) for _ in range(n))
        self.d.lit(data)
        self.literals += data
        self.run += n
        return self

    def match(self, length, dist):
        assert 3 <= length <= 258 and 1 <= dist <= self.pos
        self.d.match(length, dist)
        self._runs()
        self.entries.append((self.run, length, dist))
        self.run = 0
        return self

    def _runs(self):
        while self.run > 255:
            self.entries.append((255, 0, 1))
            self.run -= 255

    def finish(self):
        self._runs()
        if self.run:
            self.entries.append((self.run, 0, 1))
            self.run = 0
        stream, payload = self.d.eob().finish()
        return stream, payload, [lr << 24 | (dist - 1) << 9 | ln for lr, ln, dist in self.entries], bytes(self.literals)

    # ---- whole batches: 64 entries each, well under the span, so that batches tile the block as written -------------------------------
    def fast_batch(self):
        """64 near matches that all read the 200 literals in front of the first one: every source ends below the first destination."""
        start = self.pos
        for k in range(64):
            self.lit(200 if k == 0 else 1)
            self.match(4, self.pos - (start + 3 * k))
        return self

    def chain_batch(self, depth):
        """`depth` matches that each copy the output of the one before (lane k's source is lane k - 1's destination): `depth` rounds.
        The rest of the 64 entries read the literals in front of the batch."""
        start = self.pos
        self.lit(16).match(8, 16)
        for _ in range(depth - 1):
            self.lit(1).match(8, 9)                   # the match in front, byte for byte
        for k in range(64 - depth):
            self.lit(1).match(4, self.pos - (start + k % 12))
        return self


def batches_of(entries):
    """How K1b cuts a block's entries into batches: (number of entries, output bytes) each."""
    out, i = [], 0
    while i < len(entries):
        n = span = 0
        while n < 64 and i + n < len(entries) and span + (entries[i + n] >> 24) + (entries[i + n] & 511) <= SPAN_MAX:
            span += (entries[i + n] >> 24) + (entries[i + n] & 511)
            n += 1
        out.append((n, span))
        i += n
    return out


def cases():
    """[(name, deflate stream, payload, entries, literals, expected letters per batch or None, expected rounds per batch or None)];
    letters: n = no near match, f = one round under the frontier test, x = the exact rule."""
    out = []

    def add(name, t, letters=None, rounds=None):
        stream, payload, entries, literals = t.finish()
        out.append((name, stream, payload, entries, literals, letters, rounds))

    add("a_literals_only", Tokens(1).lit(700), "n", [0])                       # (three entries of <= 255 literals: one batch)
    add("b_64_independent", Tokens(2).fast_batch(), "f", [1])
    for depth in (2, 3, 63):
        add("c_chain_%d" % depth, Tokens(3 + depth).chain_batch(depth), "x", [depth])
    t = Tokens(4)
    for depth in (2, 5, 63):
        t.fast_batch().chain_batch(depth)
    add("d_alternating", t.fast_batch(), "fxfxfxf", [1, 2, 1, 5, 1, 63, 1])
    # (e) batches that the span cuts.  An entry is at most 255 + 258 = 513 bytes, so the span cannot cut a batch below 2 entries
    # (3 x 513 = 1539); a batch of ONE entry exists only as the last of a block.  Here: 2 entries (513 + 513, the third would pass
    # 1536), 63 entries (61 of 4 bytes between two of 513: 1270, a 64th of 513 would pass), 2 again, and the block's last entry alone.  The long
    # matches read the batch's own output (dist 300 < 513: near, and the second one's source is the first one's destination).
    t = Tokens(5)
    t.lit(255).match(258, 100).lit(255).match(258, 300).lit(255).match(258, 300)
    for k in range(61):
        t.lit(1).match(3, 300)
    for k in range(4):
        t.lit(255).match(258, 300)
    add("e_span_cuts", t, "xxxf", None)
    assert [n for n, _ in batches_of(out[-1][3])] == [2, 63, 2, 1]
    # (f) self-overlapping and long matches of every path directly behind a fast-path batch: dist 1, 8 (byte permutes up to 16 bytes),
    # 9 (the byte loop up to 16), 300 (plain: own lane up to 32, the cooperative copy beyond); len <= 16, 17 (the doubling loop), 258
    t = Tokens(6).fast_batch()
    for dist in (1, 8, 9, 300):
        for length in (3, 16, 17, 258):
            t.lit(1).match(length, dist)
    add("f_periodic_after_fast", t, "fx")
    # a seeded random token stream, long enough for the window to slide and for matches to reach below it (far)
    t = Tokens(7).lit(40)
    while t.pos < 24000:
        r = t.rng.random()
        length = 258 if r < 0.02 else t.rng.randrange(3, 40) if r < 0.3 else t.rng.randrange(3, 12)
        dist = t.rng.randrange(1, 12) if t.rng.random() < 0.15 else t.rng.randrange(1, min(t.pos, 6000) + 1)
        t.lit(t.rng.choice((0, 0, 1, 1, 2, 5, 20))).match(length, dist)
    add("random_tokens", t)
    return out
