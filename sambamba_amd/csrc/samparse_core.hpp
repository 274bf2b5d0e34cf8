// samparse_core.hpp -- a SAM alignment line turned into a BAM record (parseAlignmentLine, BioD bio/etc/ragel/sam_alignment.rl), the
// opposite direction of sam_core.hpp and `__host__ __device__` like it: the statements of K15 (samparse.hip) run on the CPU too
// (tests/native/samin_host.cpp: records against tests/samin_ref.py, floats against glibc's strtof).
//
// ONE walker, walk_line, goes through the fields of a line and hands every piece of the record to a sink.  Three sinks exist:
// MeasureSink adds the bytes up (sam_record_length, K15b), RecordSink writes them (sam_record_emit, K15c) and WindowSink writes those
// of them that lie inside one window of the output stream (sam_record_emit_window, K15d), so the length and the bytes come from the
// same field sequence.
//   * reads: the walker never reads a byte at or behind line + n.  The eleven mandatory fields are located first (ten tabs), every
//     field is checked against its rule of the grammar before a byte of it is used, and a line outside the grammar is kParseBad:
//     nothing of the reference's silent recovery (skip to the next tab, drop the tag, fill the qualities) is reproduced.
//   * writes: RecordSink is a fmt::RowSink (format_core.hpp: eight bytes per store, every store holds only bytes of its own record)
//     behind a count -- a put that would pass the length the record was measured with is dropped, with everything after it, and
//     the record is kParseOverrun.  So no byte outside [out, out + length) is written whatever the line holds.  WindowSink keeps the
//     same count and stores single bytes, each only after its place in the stream was found inside the window and the record.
//   * what the record needs before its variable part -- block_size, bin, n_cigar_op, l_seq -- is known before the first byte is
//     put: block_size is the measured length, the CIGAR is walked once for its count and its reference span and once more for
//     its words, l_seq is the width of the SEQ field.
//   * floats: decimal to binary32, correctly rounded (ties to even), by exact integer arithmetic -- see parse_float.
#pragma once
#include "format_core.hpp"
#include "view_core.hpp"

namespace sbx {
namespace sampc {

enum : uint32_t { kParseOk = 0, kParseBad = 1, kParseOverrun = 2 };

// The reference names of the header: name r is bytes[off[r], off[r + 1]); slots[h & (n_slots - 1)], probed linearly, holds r + 1 of
// the name with FNV-1a hash h, 0 ends the probe.  n_slots is a power of two of at least twice the names, or 0: no name resolves.
struct RefTable {
    const uint32_t* slots;
    uint32_t n_slots;
    const uint32_t* off;
    const char* bytes;
};

SBX_FMT_HD uint64_t fnv1a(const uint8_t* s, uint64_t len) {
    uint64_t h = viewc::kFnvOffset;
    for (uint64_t k = 0; k < len; ++k) { h ^= s[k]; h *= viewc::kFnvPrime; }
    return h;
}
// index of the name, or -2
SBX_FMT_HD int32_t find_ref(const RefTable& t, const uint8_t* s, uint64_t len) {
    if (!t.n_slots) return -2;
    const uint32_t mask = t.n_slots - 1u;
    for (uint32_t at = (uint32_t)fnv1a(s, len) & mask;; at = (at + 1u) & mask) {
        const uint32_t v = t.slots[at];
        if (!v) return -2;
        const uint32_t a = t.off[v - 1u], b = t.off[v];
        if ((uint64_t)(b - a) != len) continue;
        uint64_t k = 0;
        while (k < len && (uint8_t)t.bytes[a + k] == s[k]) ++k;
        if (k == len) return (int32_t)(v - 1u);
    }
}

// ---- decimal -> binary32 -------------------------------------------------------------------------------------------------------------
// The grammar's float is  [-+]? ( digit* '.'? digit+ ([eE] [-+]? digit+)? | "inf" ) | "nan"  (and "-nan", which K13 prints).  Its value
// is D * 10^E for the integer D of its significant digits.  A binary32 value, and a midpoint between two of them, has at most 113
// significant decimal digits ((2k + 1) * 2^-150 = (2k + 1) * 5^150 / 10^150 with 2k + 1 < 2^25), so the first kMaxDigits = 117 are kept
// exactly and the digits behind them only say "and a bit more" (sticky): nothing that decides a rounding lies strictly between two
// neighbouring 117-digit numbers.  Then
//     E >= 0:  value = D * 5^E * 2^E            E < 0:  value = D / 5^-E * 2^E
// Lines whose value is certainly an infinity (digits + E > 39) or certainly rounds to zero (digits + E < -45) leave first, which
// bounds E to [-162, 38] and every integer below to less than 2^480: sixteen 32-bit words.  Numerator or denominator is shifted so
// that the quotient has 27 or 28 bits, a binary long division gives it, the remainder joins the sticky bit, and the quotient is
// rounded once to the 24 bits of a normal number or to the fewer bits of a denormal one.  No floating-point arithmetic takes part.
constexpr int kBigWords = 16;
constexpr uint32_t kMaxDigits = 117;
struct Big { uint32_t w[kBigWords]; };

SBX_FMT_HD void big_set(Big& a, uint32_t v) {
    a.w[0] = v;
    for (int k = 1; k < kBigWords; ++k) a.w[k] = 0;
}
SBX_FMT_HD void big_mul_add(Big& a, uint32_t f, uint32_t add) {
    uint64_t carry = add;
    for (int k = 0; k < kBigWords; ++k) {
        const uint64_t t = (uint64_t)a.w[k] * f + carry;
        a.w[k] = (uint32_t)t;
        carry = t >> 32;
    }
}
SBX_FMT_HD void big_mul_pow5(Big& a, uint32_t s) {
    for (; s >= 13u; s -= 13u) big_mul_add(a, 1220703125u, 0u);    // 5^13
    uint32_t f = 1;
    for (; s; --s) f *= 5u;
    big_mul_add(a, f, 0u);
}
SBX_FMT_HD uint32_t big_bits(const Big& a) {
    for (int k = kBigWords - 1; k >= 0; --k)
        if (a.w[k]) return 32u * (uint32_t)k + (32u - (uint32_t)__builtin_clz(a.w[k]));
    return 0;
}
SBX_FMT_HD void big_shl(Big& a, uint32_t bits) {       // bits < 32 * kBigWords
    const int words = (int)(bits >> 5);
    const uint32_t r = bits & 31u;
    for (int k = kBigWords - 1; k >= 0; --k) {
        const uint32_t hi = k - words >= 0 ? a.w[k - words] : 0u, lo = k - words - 1 >= 0 ? a.w[k - words - 1] : 0u;
        a.w[k] = r ? (hi << r) | (lo >> (32u - r)) : hi;
    }
}
SBX_FMT_HD void big_shr1(Big& a) {
    for (int k = 0; k < kBigWords - 1; ++k) a.w[k] = (a.w[k] >> 1) | (a.w[k + 1] << 31);
    a.w[kBigWords - 1] >>= 1;
}
SBX_FMT_HD int big_cmp(const Big& a, const Big& b) {
    for (int k = kBigWords - 1; k >= 0; --k)
        if (a.w[k] != b.w[k]) return a.w[k] < b.w[k] ? -1 : 1;
    return 0;
}
SBX_FMT_HD void big_sub(Big& a, const Big& b) {        // a >= b
    uint64_t borrow = 0;
    for (int k = 0; k < kBigWords; ++k) {
        const uint64_t t = (uint64_t)a.w[k] - b.w[k] - borrow;
        a.w[k] = (uint32_t)t;
        borrow = (t >> 32) & 1u;
    }
}
SBX_FMT_HD bool big_is_zero(const Big& a) {
    uint32_t x = 0;
    for (int k = 0; k < kBigWords; ++k) x |= a.w[k];
    return x == 0;
}

SBX_FMT_HD bool is_digit(uint32_t c) { return c - '0' < 10u; }

// The bits of the float the text s[0, n) stands for; false: the text is not a float of the grammar.
SBX_FMT_HD bool parse_float(const uint8_t* s, uint64_t n, uint32_t* bits) {
    if (n == 3 && s[0] == 'n' && s[1] == 'a' && s[2] == 'n') { *bits = 0x7FC00000u; return true; }
    if (n == 4 && s[0] == '-' && s[1] == 'n' && s[2] == 'a' && s[3] == 'n') { *bits = 0xFFC00000u; return true; }
    uint64_t i = 0;
    uint32_t sign = 0;
    if (i < n && (s[i] == '-' || s[i] == '+')) { sign = s[i] == '-' ? 0x80000000u : 0u; ++i; }
    if (n - i == 3 && s[i] == 'i' && s[i + 1] == 'n' && s[i + 2] == 'f') { *bits = sign | 0x7F800000u; return true; }

    Big num;
    big_set(num, 0u);
    uint32_t nd = 0, chunk = 0, in_chunk = 0, sticky = 0;
    int64_t e10 = 0;
    uint64_t n_int = 0, n_frac = 0;
    bool point = false;
    for (; i < n; ++i) {
        const uint32_t c = s[i];
        if (c == '.' && !point) { point = true; continue; }
        if (!is_digit(c)) break;
        if (point) ++n_frac; else ++n_int;
        const uint32_t d = c - '0';
        if (nd == 0 && d == 0) { if (point) --e10; continue; }          // a zero in front of the first significant digit
        if (nd < kMaxDigits) {
            chunk = chunk * 10u + d;
            ++nd;
            if (point) --e10;
            if (++in_chunk == 9u) { big_mul_add(num, 1000000000u, chunk); chunk = 0; in_chunk = 0; }
        } else {
            sticky |= d;
            if (!point) ++e10;
        }
    }
    // digit* '.'? digit+ : the digits behind a point, or without one the digits in front, are at least one
    if (point ? n_frac == 0 : n_int == 0) return false;
    if (in_chunk) {
        uint32_t f = 1;
        for (uint32_t k = 0; k < in_chunk; ++k) f *= 10u;
        big_mul_add(num, f, chunk);
    }
    if (i < n) {
        if (s[i] != 'e' && s[i] != 'E') return false;
        ++i;
        bool neg = false;
        if (i < n && (s[i] == '-' || s[i] == '+')) { neg = s[i] == '-'; ++i; }
        if (i >= n) return false;
        int64_t ev = 0;
        for (; i < n; ++i) {
            if (!is_digit(s[i])) return false;
            if (ev < 100000000) ev = ev * 10 + (s[i] - '0');              // (saturates far beyond every exponent that matters)
        }
        e10 += neg ? -ev : ev;
    }
    if (nd == 0) { *bits = sign; return true; }
    if ((int64_t)nd + e10 > 39) { *bits = sign | 0x7F800000u; return true; }      // >= 10^39: beyond the largest float and its midpoint
    if ((int64_t)nd + e10 < -45) { *bits = sign; return true; }                   // < 10^-46: below half the smallest denormal

    Big den;
    big_set(den, 1u);
    if (e10 >= 0) big_mul_pow5(num, (uint32_t)e10); else big_mul_pow5(den, (uint32_t)-e10);
    int32_t x = (int32_t)e10;                                   // value = num / den * 2^x
    const int32_t shift = (int32_t)big_bits(den) + 27 - (int32_t)big_bits(num);
    if (shift > 0) big_shl(num, (uint32_t)shift); else big_shl(den, (uint32_t)-shift);
    x -= shift;
    constexpr uint32_t kQBits = 28;
    big_shl(den, kQBits - 1u);
    uint32_t q = 0;
    for (uint32_t bit = kQBits; bit-- > 0;) {
        if (big_cmp(num, den) >= 0) { big_sub(num, den); q |= 1u << bit; }
        if (bit) big_shr1(den);
    }
    if (!big_is_zero(num)) sticky = 1;
    // q has 27 or 28 bits; value = (q + something below one) * 2^x
    const int32_t msb = (q >> 27) ? 27 : 26, ex = msb + x;
    int32_t drop = msb - 23;
    const bool denormal = -149 - x > drop;
    if (denormal) drop = -149 - x;                              // (at most 31: the value is at least 10^-46)
    const uint64_t q64 = q, rest = q64 & ((1ull << drop) - 1ull), half = 1ull << (drop - 1);
    uint32_t kept = (uint32_t)(q64 >> drop);
    if (rest > half || (rest == half && (sticky || (kept & 1u)))) ++kept;
    uint32_t out;
    if (denormal) out = kept;                                   // (2^23 after the carry is the smallest normal number, and reads so)
    else if (ex > 127) out = 0x7F800000u;
    else out = ((uint32_t)(ex + 127) << 23) + (kept - 0x800000u);   // (a carry to 2^24 raises the exponent)
    if (out > 0x7F800000u) out = 0x7F800000u;
    *bits = sign | out;
    return true;
}

// ---- integers ------------------------------------------------------------------------------------------------------------------------
// `uint` of the grammar: 1 to 18 digits (leading zeros count)
SBX_FMT_HD bool parse_uint(const uint8_t* s, uint64_t n, uint64_t* v) {
    if (n < 1 || n > 18) return false;
    uint64_t x = 0;
    for (uint64_t k = 0; k < n; ++k) {
        if (!is_digit(s[k])) return false;
        x = x * 10u + (s[k] - '0');
    }
    *v = x;
    return true;
}
// `int`: an optional sign in front
SBX_FMT_HD bool parse_int(const uint8_t* s, uint64_t n, int64_t* v) {
    bool neg = false;
    if (n && (s[0] == '-' || s[0] == '+')) { neg = s[0] == '-'; ++s; --n; }
    uint64_t x;
    if (!parse_uint(s, n, &x)) return false;
    *v = neg ? -(int64_t)x : (int64_t)x;
    return true;
}

// reg2bin (bio/std/hts/bam/bai/bin.d:82-92) in its 32-bit arithmetic
SBX_FMT_HD uint32_t reg2bin(int32_t beg, int32_t end) {
    if (end == beg) end = (int32_t)((uint32_t)beg + 1u);
    end = (int32_t)((uint32_t)end - 1u);
    if (beg >> 14 == end >> 14) return (uint32_t)(4681 + (beg >> 14)) & 0xFFFFu;
    if (beg >> 17 == end >> 17) return (uint32_t)(585 + (beg >> 17)) & 0xFFFFu;
    if (beg >> 20 == end >> 20) return (uint32_t)(73 + (beg >> 20)) & 0xFFFFu;
    if (beg >> 23 == end >> 23) return (uint32_t)(9 + (beg >> 23)) & 0xFFFFu;
    if (beg >> 26 == end >> 26) return (uint32_t)(1 + (beg >> 26)) & 0xFFFFu;
    return 0;
}
// the bin of rule 8: pos is POS as written (1-based, 0 for none), span the reference bases of the CIGAR (32-bit, wrapping as D's int)
SBX_FMT_HD uint32_t record_bin(uint32_t pos, uint32_t span) {
    uint32_t end_pos = pos + span;
    if (end_pos == pos) ++end_pos;
    return reg2bin((int32_t)(pos - 1u), (int32_t)(end_pos - 1u));
}

// Base(char).internal_code (bio/core/base.d:42-60): "=ACMGRSVTWYHKDBN", either case; the digits 0 .. 3 are A C G T; all else N
SBX_FMT_HD uint32_t base_code(uint32_t c) {
    if (c == '=') return 0u;
    if (c - '0' < 4u) return 1u << (c - '0');
    const uint32_t k = (c & ~32u) - 'A';                         // (upper case)
    if (k >= 26u) return 15u;
    //                         N M L K J I H G F E D C B A                           Z Y X W V U T S R Q P O
    constexpr uint64_t lo = 0xF3FCFFB4FFD2E1ull, hi = 0xFAF97F865FFFull;             // a nibble each
    return (uint32_t)((k < 14u ? lo >> (4u * k) : hi >> (4u * (k - 14u))) & 15ull);
}

// ---- the three sinks -----------------------------------------------------------------------------------------------------------------
// bytes(x, k): the low k bytes of x (1 <= k <= 8, the bytes above them zero); raw: bytes of the line as they are; seq: l bases packed two
// per byte; qual: l bytes minus 33; fill: the same byte l times.
struct MeasureSink {
    uint64_t n = 0;
    SBX_FMT_HD void bytes(uint64_t, uint32_t k) { n += k; }
    SBX_FMT_HD void raw(const uint8_t*, uint64_t len) { n += len; }
    SBX_FMT_HD void seq(const uint8_t*, uint64_t l) { n += (l + 1u) / 2u; }
    SBX_FMT_HD void qual(const uint8_t*, uint64_t l) { n += l; }
    SBX_FMT_HD void fill(uint32_t, uint64_t l) { n += l; }
};

struct RecordSink {
    fmt::RowSink row;
    uint64_t cap, used;         // the measured length of the record; bytes handed to `row`
    uint32_t over;              // != 0: a put did not fit; nothing is written from there on
    SBX_FMT_HD void init(uint8_t* at, uint64_t length) { row.init(at); cap = length; used = 0; over = 0; }
    SBX_FMT_HD bool room(uint64_t k) {
        if (over || k > cap - used) { over = 1; return false; }
        used += k;
        return true;
    }
    SBX_FMT_HD void bytes(uint64_t x, uint32_t k) { if (room(k)) row.put(x, k); }
    SBX_FMT_HD void raw(const uint8_t* s, uint64_t len) {
        if (!room(len)) return;
        uint64_t i = 0;
        for (; i + 8u <= len; i += 8u) { uint64_t x; __builtin_memcpy(&x, s + i, 8); row.put(x, 8u); }
        if (i < len) {
            uint64_t x = 0;
            for (uint32_t k = 0; i + k < len; ++k) x |= (uint64_t)s[i + k] << (8u * k);
            row.put(x, (uint32_t)(len - i));
        }
    }
    SBX_FMT_HD void seq(const uint8_t* s, uint64_t l) {
        if (!room((l + 1u) / 2u)) return;
        uint64_t i = 0;
        for (; i + 16u <= l; i += 16u) {
            uint64_t x = 0;
            for (uint32_t k = 0; k < 8u; ++k) x |= (uint64_t)(base_code(s[i + 2u * k]) << 4 | base_code(s[i + 2u * k + 1u])) << (8u * k);
            row.put(x, 8u);
        }
        if (i < l) {
            uint64_t x = 0;
            uint32_t k = 0;
            for (; i + 2u * k < l; ++k) {
                uint32_t b = base_code(s[i + 2u * k]) << 4;
                if (i + 2u * k + 1u < l) b |= base_code(s[i + 2u * k + 1u]);
                x |= (uint64_t)b << (8u * k);
            }
            row.put(x, k);
        }
    }
    SBX_FMT_HD void qual(const uint8_t* s, uint64_t l) {
        if (!room(l)) return;
        uint64_t i = 0;
        for (; i + 8u <= l; i += 8u) {
            uint64_t x;
            __builtin_memcpy(&x, s + i, 8);
            row.put(x - 0x2121212121212121ull, 8u);                 // every byte is at least 33: no borrow leaves a byte
        }
        if (i < l) {
            uint64_t x = 0;
            for (uint32_t k = 0; i + k < l; ++k) x |= (uint64_t)(s[i + k] - 33u) << (8u * k);
            row.put(x, (uint32_t)(l - i));
        }
    }
    SBX_FMT_HD void fill(uint32_t v, uint64_t l) {
        if (!room(l)) return;
        const uint64_t x = 0x0101010101010101ull * (v & 0xFFu);
        uint64_t i = 0;
        for (; i + 8u <= l; i += 8u) row.put(x, 8u);
        if (i < l) row.put(x >> (8u * (8u - (uint32_t)(l - i))), (uint32_t)(l - i));
    }
};

// The record at [off, off + length) of the output stream, of which only the bytes inside the window [w0, w1) are written: stream
// byte p goes to win[p - w0].  A put is clipped to the window before a byte of it is produced, so a long SEQ or QUAL costs what lies
// inside; the stores are single bytes (at most two records of a launch take this path, K15d).  `over` as in RecordSink: a put past
// the measured length is dropped with everything after it.  wrote: the bytes stored.
struct WindowSink {
    uint8_t* win;
    uint64_t off, w0;
    uint64_t lo, hi;            // bytes [lo, hi) of the record lie inside the window (lo >= hi: none)
    uint64_t cap, used, wrote;
    uint32_t over;
    SBX_FMT_HD void init(uint8_t* window, uint64_t window_from, uint64_t window_to, uint64_t at, uint64_t length) {
        win = window; off = at; w0 = window_from; cap = length; used = 0; wrote = 0; over = 0;
        const uint64_t a = at > window_from ? at : window_from, b = at + length < window_to ? at + length : window_to;
        lo = a < b ? a - at : 0;
        hi = a < b ? b - at : 0;
    }
    // A put of k bytes: its bytes [*a, *b) lie inside, byte *a goes to *dst.  false: none does, or the put did not fit.
    SBX_FMT_HD bool clip(uint64_t k, uint64_t* a, uint64_t* b, uint8_t** dst) {
        if (over || k > cap - used) { over = 1; return false; }
        const uint64_t at = used;
        used += k;
        const uint64_t s = at > lo ? at : lo, e = at + k < hi ? at + k : hi;
        if (s >= e) return false;
        *a = s - at;
        *b = e - at;
        *dst = win + (off + s - w0);                            // (s >= lo: off + s >= w0)
        wrote += e - s;
        return true;
    }
    SBX_FMT_HD void bytes(uint64_t x, uint32_t k) {
        uint64_t a, b;
        uint8_t* d;
        if (clip(k, &a, &b, &d)) for (uint64_t j = a; j < b; ++j) d[j - a] = (uint8_t)(x >> (8u * j));
    }
    SBX_FMT_HD void raw(const uint8_t* s, uint64_t len) {
        uint64_t a, b;
        uint8_t* d;
        if (clip(len, &a, &b, &d)) for (uint64_t j = a; j < b; ++j) d[j - a] = s[j];
    }
    SBX_FMT_HD void seq(const uint8_t* s, uint64_t l) {
        uint64_t a, b;
        uint8_t* d;
        if (clip((l + 1u) / 2u, &a, &b, &d))
            for (uint64_t j = a; j < b; ++j) {
                uint32_t v = base_code(s[2u * j]) << 4;
                if (2u * j + 1u < l) v |= base_code(s[2u * j + 1u]);
                d[j - a] = (uint8_t)v;
            }
    }
    SBX_FMT_HD void qual(const uint8_t* s, uint64_t l) {
        uint64_t a, b;
        uint8_t* d;
        if (clip(l, &a, &b, &d)) for (uint64_t j = a; j < b; ++j) d[j - a] = (uint8_t)(s[j] - 33u);
    }
    SBX_FMT_HD void fill(uint32_t v, uint64_t l) {
        uint64_t a, b;
        uint8_t* d;
        if (clip(l, &a, &b, &d)) for (uint64_t j = a; j < b; ++j) d[j - a] = (uint8_t)v;
    }
};

// ---- the walker ----------------------------------------------------------------------------------------------------------------------
SBX_FMT_HD bool is_graph(uint32_t c) { return c - 33u < 94u; }                    // [!-~]
SBX_FMT_HD bool is_alpha(uint32_t c) { return (c | 32u) - 'a' < 26u; }
SBX_FMT_HD bool is_xdigit(uint32_t c) { return is_digit(c) || (c | 32u) - 'a' < 6u; }

// RNAME / RNEXT that is a name: [!-()+-<>-~][!-~]* -- graphic bytes, the first neither '*' nor '='
SBX_FMT_HD bool ref_name_ok(const uint8_t* s, uint64_t n) {
    if (!n || s[0] == '*' || s[0] == '=') return false;
    for (uint64_t k = 0; k < n; ++k) if (!is_graph(s[k])) return false;
    return true;
}

// "MIDNSHP=X" -> 0 .. 8; 15: no operation
SBX_FMT_HD uint32_t cigar_op_code(uint32_t c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return 15;
    }
}
// One operation at s[*i ...): digits (1 .. 18, value below 2^28) and its letter.  Advances *i behind it.
SBX_FMT_HD bool next_cigar_op(const uint8_t* s, uint64_t n, uint64_t* i, uint32_t* raw) {
    uint64_t k = *i, v = 0;
    while (k < n && is_digit(s[k])) {
        if (k - *i >= 18u) return false;
        v = v * 10u + (s[k] - '0');
        ++k;
    }
    if (k == *i || k >= n || v >= (1ull << 28)) return false;
    const uint32_t op = cigar_op_code(s[k]);
    if (op == 15u) return false;
    *raw = (uint32_t)v << 4 | op;
    *i = k + 1u;
    return true;
}

// the integer of a tag of type i in the smallest type (set_integervalue): the type letter and the bytes of the value
SBX_FMT_HD bool tag_integer(int64_t v, uint32_t* type, uint32_t* size) {
    if (v < 0) {
        if (v >= -128) { *type = 'c'; *size = 1; }
        else if (v >= -32768) { *type = 's'; *size = 2; }
        else if (v >= -2147483648ll) { *type = 'i'; *size = 4; }
        else return false;
    } else {
        if (v <= 255) { *type = 'C'; *size = 1; }
        else if (v <= 65535) { *type = 'S'; *size = 2; }
        else if (v <= 4294967295ll) { *type = 'I'; *size = 4; }
        else return false;
    }
    return true;
}
// an element of a B array of integers fits its type (to!byte and the like); *size: its bytes
SBX_FMT_HD bool array_integer_fits(uint32_t sub, int64_t v, uint32_t* size) {
    switch (sub) {
        case 'c': *size = 1; return v >= -128 && v <= 127;
        case 'C': *size = 1; return v >= 0 && v <= 255;
        case 's': *size = 2; return v >= -32768 && v <= 32767;
        case 'S': *size = 2; return v >= 0 && v <= 65535;
        case 'i': *size = 4; return v >= -2147483648ll && v <= 2147483647ll;
        case 'I': *size = 4; return v >= 0 && v <= 4294967295ll;
        default: return false;
    }
}

// One optional field s[0, n): [A-Za-z][A-Za-z0-9]:T:value
template <class Sink>
SBX_FMT_HD bool walk_tag(const uint8_t* s, uint64_t n, Sink& out) {
    if (n < 6u || !is_alpha(s[0]) || !(is_alpha(s[1]) || is_digit(s[1])) || s[2] != ':' || s[4] != ':') return false;
    const uint64_t key = (uint64_t)s[0] | (uint64_t)s[1] << 8;
    const uint8_t* v = s + 5;
    const uint64_t vn = n - 5u;
    switch (s[3]) {
        case 'A':
            if (vn != 1u || !is_graph(v[0])) return false;
            out.bytes(key | (uint64_t)'A' << 16 | (uint64_t)v[0] << 24, 4u);
            return true;
        case 'i': {
            int64_t x;
            uint32_t type, size;
            if (!parse_int(v, vn, &x) || !tag_integer(x, &type, &size)) return false;
            out.bytes(key | (uint64_t)type << 16, 3u);
            out.bytes((uint64_t)x & (size == 4u ? 0xFFFFFFFFull : size == 2u ? 0xFFFFull : 0xFFull), size);
            return true;
        }
        case 'f': {
            uint32_t bits;
            if (!parse_float(v, vn, &bits)) return false;
            out.bytes(key | (uint64_t)'f' << 16 | (uint64_t)bits << 24, 7u);
            return true;
        }
        case 'Z':
            for (uint64_t k = 0; k < vn; ++k) if (v[k] != ' ' && !is_graph(v[k])) return false;
            out.bytes(key | (uint64_t)'Z' << 16, 3u);
            out.raw(v, vn);
            out.bytes(0, 1u);
            return true;
        case 'H':
            for (uint64_t k = 0; k < vn; ++k) if (!is_xdigit(v[k])) return false;
            out.bytes(key | (uint64_t)'H' << 16, 3u);
            out.raw(v, vn);
            out.bytes(0, 1u);
            return true;
        case 'B': {
            const uint32_t sub = v[0];
            if (vn < 2u || v[1] != ',') return false;
            if (sub != 'c' && sub != 'C' && sub != 's' && sub != 'S' && sub != 'i' && sub != 'I' && sub != 'f') return false;
            // the elements: one behind every comma; "B:c," alone, which K13 prints for an empty array, has none
            uint64_t count = 0;
            if (vn > 2u) for (uint64_t k = 1; k < vn; ++k) count += v[k] == ',';
            if (count > 0xFFFFFFFFull) return false;
            out.bytes(key | (uint64_t)'B' << 16 | (uint64_t)sub << 24 | count << 32, 8u);
            uint64_t a = 2;
            for (uint64_t e = 0; e < count; ++e) {
                uint64_t b = a;
                while (b < vn && v[b] != ',') ++b;
                if (sub == 'f') {
                    uint32_t bits;
                    if (!parse_float(v + a, b - a, &bits)) return false;
                    out.bytes(bits, 4u);
                } else {
                    int64_t x;
                    uint32_t size;
                    if (!parse_int(v + a, b - a, &x) || !array_integer_fits(sub, x, &size)) return false;
                    out.bytes((uint64_t)x & (size == 4u ? 0xFFFFFFFFull : size == 2u ? 0xFFFFull : 0xFFull), size);
                }
                a = b + 1u;
            }
            return true;
        }
        default: return false;
    }
}

// The record of the line s[0, n) (no '\n'), its block_size word first.  block_size: the value of that word (the measured length
// minus four; the measuring sink does not look at it).
template <class Sink>
SBX_FMT_HD uint32_t walk_line(const uint8_t* s, uint64_t n, const RefTable& refs, uint32_t block_size, Sink& out) {
    // the eleven mandatory fields: field k is s[fb[k], fe[k])
    uint64_t fb[11], fe[11];
    uint64_t at = 0;
    for (int k = 0; k < 11; ++k) {
        fb[k] = at;
        while (at < n && s[at] != '\t') ++at;
        fe[k] = at;
        if (k < 10) {
            if (at >= n) return kParseBad;
            ++at;
        }
    }
    const uint64_t tags_at = at;                                   // n, or the tab in front of the first optional field

    // 1 QNAME
    const uint64_t l_name = fe[0] - fb[0];
    if (l_name < 1u || l_name > 254u) return kParseBad;
    for (uint64_t k = fb[0]; k < fe[0]; ++k) if (!is_graph(s[k]) || s[k] == '@') return kParseBad;
    // 2 FLAG, 4 POS, 5 MAPQ, 8 PNEXT, 9 TLEN
    uint64_t flag, pos, mapq, pnext;
    int64_t tlen;
    if (!parse_uint(s + fb[1], fe[1] - fb[1], &flag) || flag > 65535u) return kParseBad;
    if (!parse_uint(s + fb[3], fe[3] - fb[3], &pos) || pos > 0x7FFFFFFFull) return kParseBad;
    if (!parse_uint(s + fb[4], fe[4] - fb[4], &mapq) || mapq > 255u) return kParseBad;
    if (!parse_uint(s + fb[7], fe[7] - fb[7], &pnext) || pnext > 0x7FFFFFFFull) return kParseBad;
    if (!parse_int(s + fb[8], fe[8] - fb[8], &tlen) || tlen < -2147483648ll || tlen > 2147483647ll) return kParseBad;
    // 3 RNAME, 7 RNEXT
    int32_t ref = -1, mate_ref = -1;
    if (!(fe[2] - fb[2] == 1u && s[fb[2]] == '*')) {
        if (!ref_name_ok(s + fb[2], fe[2] - fb[2])) return kParseBad;
        ref = find_ref(refs, s + fb[2], fe[2] - fb[2]);
        if (ref < 0) return kParseBad;
    }
    if (fe[6] - fb[6] == 1u && s[fb[6]] == '=') mate_ref = ref;
    else if (!(fe[6] - fb[6] == 1u && s[fb[6]] == '*')) {
        if (!ref_name_ok(s + fb[6], fe[6] - fb[6])) return kParseBad;
        mate_ref = find_ref(refs, s + fb[6], fe[6] - fb[6]);
        if (mate_ref < 0) return kParseBad;
    }
    // 6 CIGAR, first time: the number of operations and the reference bases they consume
    const uint8_t* cig = s + fb[5];
    const uint64_t cig_n = fe[5] - fb[5];
    uint32_t n_cigar = 0, span = 0;
    if (!(cig_n == 1u && cig[0] == '*')) {
        uint64_t i = 0;
        while (i < cig_n) {
            uint32_t raw;
            if (!next_cigar_op(cig, cig_n, &i, &raw) || n_cigar == 65535u) return kParseBad;
            ++n_cigar;
            const uint32_t op = raw & 15u;
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += raw >> 4;      // is_reference_consuming: M D N = X
        }
        if (!n_cigar) return kParseBad;
    }
    // 10 SEQ, 11 QUAL
    const uint8_t* seq = s + fb[9];
    uint64_t l_seq = fe[9] - fb[9];
    if (l_seq == 1u && seq[0] == '*') l_seq = 0;
    else {
        if (!l_seq || l_seq > 0x7FFFFFFFull) return kParseBad;
        for (uint64_t k = 0; k < l_seq; ++k) if (!is_alpha(seq[k]) && seq[k] != '=' && seq[k] != '.') return kParseBad;
    }
    const uint8_t* qual = s + fb[10];
    const uint64_t l_qual = fe[10] - fb[10];
    if (!l_qual) return kParseBad;
    const bool qual_star = l_qual == 1u && qual[0] == '*';
    if (!qual_star) {
        if (l_qual != l_seq) return kParseBad;
        for (uint64_t k = 0; k < l_qual; ++k) if (!is_graph(qual[k])) return kParseBad;
    }

    out.bytes((uint64_t)block_size | (uint64_t)(uint32_t)ref << 32, 8u);
    out.bytes((uint64_t)(uint32_t)((uint32_t)pos - 1u) | (uint64_t)((uint32_t)l_name + 1u) << 32 | mapq << 40 |
                  (uint64_t)record_bin((uint32_t)pos, span) << 48, 8u);
    out.bytes((uint64_t)n_cigar | flag << 16 | l_seq << 32, 8u);
    out.bytes((uint64_t)(uint32_t)mate_ref | (uint64_t)(uint32_t)((uint32_t)pnext - 1u) << 32, 8u);
    out.bytes((uint64_t)(uint32_t)(int32_t)tlen, 4u);
    out.raw(s + fb[0], l_name);
    out.bytes(0, 1u);
    for (uint64_t i = 0; n_cigar && i < cig_n;) {
        uint32_t raw;
        if (!next_cigar_op(cig, cig_n, &i, &raw)) return kParseBad;
        out.bytes(raw, 4u);
    }
    if (l_seq) out.seq(seq, l_seq);
    // a lone '*': no qualities for no bases; the quality 9 ('*' - 33) of one base; 0xFF for every base of more (check_qual_length)
    if (!qual_star || l_seq == 1u) out.qual(qual, l_seq);
    else if (l_seq) out.fill(0xFFu, l_seq);

    // ('\t' optionalfield)*
    at = tags_at;
    while (at < n) {
        const uint64_t a = at + 1u;                                // behind the tab
        uint64_t b = a;
        while (b < n && s[b] != '\t') ++b;
        if (!walk_tag(s + a, b - a, out)) return kParseBad;
        at = b;
    }
    return kParseOk;
}

// kParseOk and *length = the bytes of the record (block_size word included), or kParseBad.  A record whose block_size would not be
// a positive int is bad too.
SBX_FMT_HD uint32_t sam_record_length(const uint8_t* line, uint64_t n, const RefTable& refs, uint64_t* length) {
    MeasureSink s;
    const uint32_t st = walk_line(line, n, refs, 0u, s);
    *length = s.n;
    if (st == kParseOk && s.n > 0x7FFFFFF0ull) return kParseBad;
    return st;
}

// Writes the record to out[0, length), `length` as sam_record_length gave it.  kParseOverrun when the walk wanted to write more or
// ended with fewer bytes (then what was written is a prefix of the record and no byte lies outside out[0, length)).
SBX_FMT_HD uint32_t sam_record_emit(const uint8_t* line, uint64_t n, const RefTable& refs, uint8_t* out, uint64_t length) {
    RecordSink s;
    s.init(out, length);
    const uint32_t st = walk_line(line, n, refs, (uint32_t)(length - 4u), s);
    s.row.finish();
    if (st != kParseOk) return st;
    return s.over || s.used != length ? kParseOverrun : kParseOk;
}

// The same record as a part of the output stream: it lies at [off, off + length) there and only its bytes inside [w0, w1) are
// written, stream byte p to window[p - w0]; *wrote receives their number ((min(off + length, w1) - max(off, w0)) for a record
// that is as long as it was measured).  The status is sam_record_emit's, whatever the window.
SBX_FMT_HD uint32_t sam_record_emit_window(const uint8_t* line, uint64_t n, const RefTable& refs, uint64_t off, uint64_t length, uint8_t* window,
                                           uint64_t w0, uint64_t w1, uint64_t* wrote) {
    WindowSink s;
    s.init(window, w0, w1, off, length);
    const uint32_t st = walk_line(line, n, refs, (uint32_t)(length - 4u), s);
    *wrote = s.wrote;
    if (st != kParseOk) return st;
    return s.over || s.used != length ? kParseOverrun : kParseOk;
}

// the bytes of the line that starts at text[at] of a text of `size` bytes: up to the '\n' or the end
SBX_FMT_HD uint64_t line_bytes(const uint8_t* text, uint64_t at, uint64_t size) {
    uint64_t e = at;
    while (e < size && text[e] != '\n') ++e;
    return e - at;
}

}  // namespace sampc
}  // namespace sbx

// ---- host only ----
#include <string>
#include <vector>

namespace sbx {
namespace sampc {

// the slots of a RefTable over these names (the first of equal names keeps its place); empty for no names
inline std::vector<uint32_t> ref_table_slots(const std::vector<std::string>& names) {
    std::vector<uint32_t> slots;
    if (names.empty()) return slots;
    size_t n_slots = 2;
    while (n_slots < 2 * names.size()) n_slots *= 2;
    slots.assign(n_slots, 0u);
    for (size_t r = 0; r < names.size(); ++r) {
        bool seen = false;
        for (size_t q = 0; q < r && !seen; ++q) seen = names[q] == names[r];
        if (seen) continue;
        size_t at = (size_t)((uint32_t)fnv1a((const uint8_t*)names[r].data(), names[r].size()) & (uint32_t)(n_slots - 1));
        while (slots[at]) at = (at + 1) & (n_slots - 1);
        slots[at] = (uint32_t)r + 1u;
    }
    return slots;
}

}  // namespace sampc
}  // namespace sbx
