// sam_core.hpp -- the SAM line of a BAM record (BamRead.toSam, BioD bio/std/hts/bam/read.d:695-760; TagValue.toSam, tagvalue.d:468-505;
// CigarOperation.toSam, cigar.d:103-111), `__host__ __device__` so that the statements of K13 (sam.hip) run on the CPU too
// (tests/native/sam_host.cpp: lines against tests/sam_ref.py, %g against glibc's snprintf).
//
// ONE walker, walk_record, goes through the fields of a record and hands every piece of text to a sink.  Two sinks exist: LengthSink
// adds the bytes up (sam_line_length, K13a) and LineSink writes them (sam_line_emit, K13b), so the length and the bytes come from
// the same field sequence.
//   * reads: the walker never reads a byte at or behind rec + len.  The fixed part is checked as a whole (36 bytes, then name, CIGAR,
//     sequence and qualities against len); the tag walk checks every tag before it reads it.  A record that breaks a bound, names
//     a reference outside [-1, n_ref), has a tag of unknown type or a Z / H without NUL is kSamBad, and nothing is read behind
//     the place that told.
//   * writes: LineSink is a fmt::RowSink (format_core.hpp: eight bytes per store, every store holds only bytes of its own row) behind a
//     count -- a put that would pass the length the line was measured with is dropped, with everything after it, and the line is
//     kSamOverrun.  So no byte outside [line, line + length) is written whatever the record holds.
//   * sequence: four packed bytes -> eight characters -> one store; qualities: + 33 on eight bytes at a time (the carry of a byte is
//     kept out of its neighbour, (q + 33) & 0xFF as the reference's cast(char) does).
//   * %g of a float (format.d:122 hands the value, widened to double, to snprintf("%g")): exact integer arithmetic, see g_digits.
#pragma once
#include "format_core.hpp"

namespace sbx {
namespace samc {

enum : uint32_t { kSamOk = 0, kSamBad = 1, kSamOverrun = 2 };

// the reference names: name r is bytes[off[r], off[r + 1])
struct RefNames {
    const uint32_t* off;
    const char* bytes;
    int32_t n;
};

SBX_FMT_HD uint32_t rd16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
SBX_FMT_HD uint32_t rd32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
SBX_FMT_HD uint64_t rd64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

// ---- %g ----------------------------------------------------------------------------------------------------------------------------
// A finite float is m * 2^e, m < 2^24, -149 <= e <= 104.  Its six significant digits are round-half-even(m * 2^e * 10^s) for the s
// that brings the product into [10^5, 10^6): a quotient num / den of two integers,
//     s >= 0:  m * 5^s * 2^max(e + s, 0)  /  2^max(-(e + s), 0)            s < 0:  m * 2^max(e + s, 0)  /  5^-s * 2^max(-(e + s), 0)
// with num < 2^128 and den < 2^100 (s <= 50 for the smallest denormal, s >= -33 for the largest float), held in six 32-bit words.
// The quotient (< 10^8 even when the first guess of s is off by two) comes out of a binary long division, the remainder decides
// the rounding exactly.
constexpr int kBigWords = 6;
struct Big { uint32_t w[kBigWords]; };

SBX_FMT_HD void big_set(Big& a, uint32_t v) {
    a.w[0] = v;
    for (int k = 1; k < kBigWords; ++k) a.w[k] = 0;
}
SBX_FMT_HD void big_mul_small(Big& a, uint32_t f) {
    uint64_t carry = 0;
    for (int k = 0; k < kBigWords; ++k) {
        const uint64_t t = (uint64_t)a.w[k] * f + carry;
        a.w[k] = (uint32_t)t;
        carry = t >> 32;
    }
}
SBX_FMT_HD void big_mul_pow5(Big& a, uint32_t s) {
    for (; s >= 13u; s -= 13u) big_mul_small(a, 1220703125u);      // 5^13
    uint32_t f = 1;
    for (; s; --s) f *= 5u;
    big_mul_small(a, f);
}
SBX_FMT_HD void big_shl(Big& a, uint32_t bits) {       // bits < 32 * kBigWords
    for (int r = 0; r < kBigWords - 1; ++r) {
        if (bits >= 32u) {
            for (int k = kBigWords - 1; k > 0; --k) a.w[k] = a.w[k - 1];
            a.w[0] = 0;
            bits -= 32u;
        }
    }
    if (bits) {
        for (int k = kBigWords - 1; k > 0; --k) a.w[k] = (a.w[k] << bits) | (a.w[k - 1] >> (32u - bits));
        a.w[0] <<= bits;
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

// round-half-even(m * 2^e * 10^s); *floor_q: the quotient before rounding
SBX_FMT_HD uint32_t scaled_digits(uint32_t m, int32_t e, int32_t s, uint32_t* floor_q) {
    constexpr uint32_t kQBits = 27;                    // 10^8 < 2^27
    Big num, den;
    big_set(num, m);
    big_set(den, 1u);
    if (s >= 0) big_mul_pow5(num, (uint32_t)s); else big_mul_pow5(den, (uint32_t)-s);
    const int32_t sh = e + s;
    if (sh >= 0) big_shl(num, (uint32_t)sh); else big_shl(den, (uint32_t)-sh);
    big_shl(den, kQBits - 1u);
    uint32_t q = 0;
    for (uint32_t bit = kQBits; bit-- > 0;) {
        if (big_cmp(num, den) >= 0) { big_sub(num, den); q |= 1u << bit; }
        if (bit) big_shr1(den);
    }
    *floor_q = q;
    big_shl(num, 1u);                                  // 2 * remainder against the divisor
    const int c = big_cmp(num, den);
    return q + ((c > 0 || (c == 0 && (q & 1u))) ? 1u : 0u);
}

// up to sixteen bytes of text, built in two registers
struct Text16 {
    uint64_t lo = 0, hi = 0;
    uint32_t n = 0;
    SBX_FMT_HD void push(uint32_t c) {
        if (n < 8u) lo |= (uint64_t)c << (8u * n); else hi |= (uint64_t)c << (8u * (n - 8u));
        ++n;
    }
};

// snprintf("%g", (double)f) of the float with these bits, as glibc prints it (at most 12 bytes)
SBX_FMT_HD Text16 g_format(uint32_t bits) {
    Text16 t;
    const uint32_t be = (bits >> 23) & 0xFFu, frac = bits & 0x7FFFFFu;
    if (bits >> 31) t.push('-');
    if (be == 0xFFu) {
        if (frac) { t.push('n'); t.push('a'); t.push('n'); } else { t.push('i'); t.push('n'); t.push('f'); }
        return t;
    }
    if (be == 0 && frac == 0) { t.push('0'); return t; }
    const uint32_t m = be ? frac | 0x800000u : frac;
    const int32_t e = (be ? (int32_t)be : 1) - 150;
    // floor(log10) of the value from floor(log2) (315653 / 2^20 = log10(2) - 3e-8); the loop below mends a guess that is off
    uint32_t top = 0;
    for (uint32_t x = m; x > 1u; x >>= 1) ++top;
    int32_t x10 = ((e + (int32_t)top) * 315653) >> 20;
    uint32_t q = 0, fq = 0;
    for (int round = 0; round < 4; ++round) {
        q = scaled_digits(m, e, 5 - x10, &fq);
        if (fq >= 1000000u) ++x10;
        else if (fq < 100000u) --x10;
        else break;
    }
    if (q >= 1000000u) { q = 100000u; ++x10; }         // 999999.5 and above: the carry makes a seventh digit
    uint32_t d[6];
    for (int k = 5; k >= 0; --k) { d[k] = q % 10u; q /= 10u; }
    int32_t p = 6;                                     // significant digits that are left once the trailing zeros are gone
    while (p > 1 && d[p - 1] == 0) --p;
    if (x10 < -4 || x10 >= 6) {
        t.push('0' + d[0]);
        if (p > 1) t.push('.');
        for (int32_t k = 1; k < p; ++k) t.push('0' + d[k]);
        t.push('e');
        t.push(x10 < 0 ? '-' : '+');
        const uint32_t ax = (uint32_t)(x10 < 0 ? -x10 : x10);
        t.push('0' + ax / 10u);
        t.push('0' + ax % 10u);
    } else if (x10 >= 0) {
        for (int32_t k = 0; k <= x10; ++k) t.push('0' + d[k]);
        if (p > x10 + 1) t.push('.');
        for (int32_t k = x10 + 1; k < p; ++k) t.push('0' + d[k]);
    } else {
        t.push('0');
        t.push('.');
        for (int32_t k = -1; k > x10; --k) t.push('0');
        for (int32_t k = 0; k < p; ++k) t.push('0' + d[k]);
    }
    return t;
}

// ---- the two sinks -------------------------------------------------------------------------------------------------------------------
// bytes(x, k): the low k bytes of x (1 <= k <= 8, the bytes above them zero); u32 / i32: decimal; str: bytes from memory; seq / qual:
// the two long fields; f32: %g.
struct LengthSink {
    uint64_t n = 0;
    SBX_FMT_HD void bytes(uint64_t, uint32_t k) { n += k; }
    SBX_FMT_HD void u32(uint32_t v) { n += fmt::n_digits32(v); }
    SBX_FMT_HD void i32(int32_t v) { n += v < 0 ? 1u + fmt::n_digits32(0u - (uint32_t)v) : fmt::n_digits32((uint32_t)v); }
    SBX_FMT_HD void str(const uint8_t*, uint32_t len) { n += len; }
    SBX_FMT_HD void seq(const uint8_t*, uint32_t l_seq) { n += l_seq; }
    SBX_FMT_HD void qual(const uint8_t*, uint32_t l_seq) { n += l_seq; }
    SBX_FMT_HD void f32(uint32_t bits) { n += g_format(bits).n; }
};

struct LineSink {
    fmt::RowSink row;
    uint64_t cap, used;         // the measured length of the line; bytes handed to `row`
    uint32_t over;              // != 0: a put did not fit; nothing is written from there on
    SBX_FMT_HD void init(uint8_t* at, uint64_t length) { row.init(at); cap = length; used = 0; over = 0; }
    SBX_FMT_HD bool room(uint64_t k) {
        if (over || used + k > cap) { over = 1; return false; }
        used += k;
        return true;
    }
    SBX_FMT_HD void bytes(uint64_t x, uint32_t k) { if (room(k)) row.put(x, k); }
    SBX_FMT_HD void u32(uint32_t v) {
        const uint32_t nd = fmt::n_digits32(v);
        if (!room(nd)) return;
        if (v < 10000u) { row.put((uint64_t)(fmt::dec4(v) >> (8u * (4u - nd))), nd); return; }
        const uint32_t hi = v / 10000u, lo = v - hi * 10000u;
        if (hi < 10000u) row.put((uint64_t)(fmt::dec4(hi) >> (8u * (8u - nd))), nd - 4u);
        else {
            const uint32_t top = hi / 10000u, mid = hi - top * 10000u;
            row.put((uint64_t)(fmt::dec4(top) >> (8u * (12u - nd))), nd - 8u);
            row.put((uint64_t)fmt::dec4(mid), 4u);
        }
        row.put((uint64_t)fmt::dec4(lo), 4u);
    }
    SBX_FMT_HD void i32(int32_t v) {
        if (v < 0) { bytes('-', 1u); u32(0u - (uint32_t)v); } else u32((uint32_t)v);
    }
    SBX_FMT_HD void str(const uint8_t* s, uint32_t len) { if (room(len)) row.str((const char*)s, len); }
    // "=ACMGRSVTWYHKDBN"[nibble], the high nibble of a byte first
    SBX_FMT_HD static uint64_t base_char(uint32_t nib) {
        constexpr uint64_t lo = 0x565352474D43413Dull, hi = 0x4E42444B48595754ull;    // "=ACMGRSV", "TWYHKDBN" in memory order
        return (((nib & 8u) ? hi : lo) >> (8u * (nib & 7u))) & 0xFFull;
    }
    SBX_FMT_HD void seq(const uint8_t* s, uint32_t l_seq) {
        if (!room(l_seq)) return;
        uint32_t i = 0;                                 // bases done; i is even in the loops
        for (; i + 8u <= l_seq; i += 8u) {
            const uint32_t w = rd32(s + (i >> 1));
            uint64_t x = 0;
            for (uint32_t k = 0; k < 4u; ++k) {
                const uint32_t b = (w >> (8u * k)) & 0xFFu;
                x |= (base_char(b >> 4) | (base_char(b & 15u) << 8)) << (16u * k);
            }
            row.put(x, 8u);
        }
        if (i < l_seq) {
            uint64_t x = 0;
            for (uint32_t k = 0; i + k < l_seq; ++k) {
                const uint32_t b = s[(i + k) >> 1];
                x |= base_char((k & 1u) ? b & 15u : b >> 4) << (8u * k);
            }
            row.put(x, l_seq - i);
        }
    }
    SBX_FMT_HD void qual(const uint8_t* s, uint32_t l_seq) {
        if (!room(l_seq)) return;
        constexpr uint64_t k7f = 0x7F7F7F7F7F7F7F7Full, k33 = 0x2121212121212121ull;
        uint32_t i = 0;
        for (; i + 8u <= l_seq; i += 8u) {
            const uint64_t x = rd64(s + i);
            row.put(((x & k7f) + k33) ^ (x & ~k7f), 8u);       // every byte + 33 mod 256: the top bits are added without carry
        }
        if (i < l_seq) {
            uint64_t x = 0;
            for (uint32_t k = 0; i + k < l_seq; ++k) x |= (uint64_t)((s[i + k] + 33u) & 0xFFu) << (8u * k);
            row.put(x, l_seq - i);
        }
    }
    SBX_FMT_HD void f32(uint32_t bits) {
        const Text16 t = g_format(bits);
        if (!room(t.n)) return;
        row.put(t.lo, t.n < 8u ? t.n : 8u);
        if (t.n > 8u) row.put(t.hi, t.n - 8u);
    }
};

// ---- the walker ----------------------------------------------------------------------------------------------------------------------
// bytes of one element of a B array / of a scalar tag of this type; 0: no such type
SBX_FMT_HD uint32_t scalar_size(uint32_t type) {
    return type == 'c' || type == 'C' ? 1u : type == 's' || type == 'S' ? 2u : type == 'i' || type == 'I' || type == 'f' ? 4u : 0u;
}
template <class Sink>
SBX_FMT_HD void put_scalar(Sink& s, uint32_t type, const uint8_t* p) {
    switch (type) {
        case 'c': s.i32((int8_t)p[0]); break;
        case 'C': s.u32(p[0]); break;
        case 's': s.i32((int16_t)rd16(p)); break;
        case 'S': s.u32(rd16(p)); break;
        case 'i': s.i32((int32_t)rd32(p)); break;
        case 'I': s.u32(rd32(p)); break;
        default: s.f32(rd32(p)); break;
    }
}
template <class Sink>
SBX_FMT_HD void put_ref_name(Sink& s, const RefNames& refs, int32_t id) {
    const uint32_t a = refs.off[id];
    s.str((const uint8_t*)refs.bytes + a, refs.off[id + 1] - a);
}

// The line of the record at rec (its block_size word first; len = block_size + 4 bytes belong to it), the '\n' included.
template <class Sink>
SBX_FMT_HD uint32_t walk_record(const uint8_t* rec, uint64_t len, const RefNames& refs, Sink& s) {
    if (len < 36u) return kSamBad;
    const int32_t ref = (int32_t)rd32(rec + 4), pos = (int32_t)rd32(rec + 8);
    const uint32_t l_name = rec[12], mapq = rec[13], fnc = rd32(rec + 16);
    const uint32_t n_cigar = fnc & 0xFFFFu, flag = fnc >> 16;
    const int32_t l_seq_s = (int32_t)rd32(rec + 20), mate_ref = (int32_t)rd32(rec + 24), mate_pos = (int32_t)rd32(rec + 28);
    const int32_t tlen = (int32_t)rd32(rec + 32);
    if (l_seq_s < 0) return kSamBad;
    const uint32_t l_seq = (uint32_t)l_seq_s;
    const uint64_t cigar_at = 36ull + l_name, seq_at = cigar_at + 4ull * n_cigar, qual_at = seq_at + ((uint64_t)l_seq + 1u) / 2u;
    const uint64_t tags_at = qual_at + l_seq;
    if (tags_at > len) return kSamBad;
    if (ref < -1 || ref >= refs.n || mate_ref < -1 || mate_ref >= refs.n) return kSamBad;

    if (l_name > 1u) s.str(rec + 36, l_name - 1u);
    s.bytes('\t', 1u);
    s.u32(flag);
    s.bytes('\t', 1u);
    if (ref == -1) s.bytes('*', 1u); else put_ref_name(s, refs, ref);
    s.bytes('\t', 1u);
    s.i32((int32_t)((uint32_t)pos + 1u));              // (int arithmetic that wraps, as D's)
    s.bytes('\t', 1u);
    s.u32(mapq);
    s.bytes('\t', 1u);
    if (n_cigar == 0) s.bytes('*', 1u);
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t raw = rd32(rec + cigar_at + 4ull * k), op = raw & 15u;
        s.u32(raw >> 4);
        // "MIDNSHP=X???????"[op]
        s.bytes(op < 8u ? (0x3D5048534E44494Dull >> (8u * op)) & 0xFFull : op == 8u ? (uint64_t)'X' : (uint64_t)'?', 1u);
    }
    s.bytes('\t', 1u);
    if (mate_ref == -1) s.bytes('*', 1u);
    else if (mate_ref == ref) s.bytes('=', 1u);
    else put_ref_name(s, refs, mate_ref);
    s.bytes('\t', 1u);
    s.i32((int32_t)((uint32_t)mate_pos + 1u));
    s.bytes('\t', 1u);
    s.i32(tlen);
    s.bytes('\t', 1u);
    if (l_seq == 0) s.bytes((uint64_t)'*' | (uint64_t)'\t' << 8 | (uint64_t)'*' << 16, 3u);
    else {
        s.seq(rec + seq_at, l_seq);
        s.bytes('\t', 1u);
        if (rec[qual_at] == 0xFFu) s.bytes('*', 1u); else s.qual(rec + qual_at, l_seq);
    }

    // the tags: every read is preceded by the check that its bytes belong to the record
    uint64_t p = tags_at;
    while (p < len) {
        if (p + 3u > len) return kSamBad;
        const uint32_t type = rec[p + 2];
        s.bytes((uint64_t)'\t' | (uint64_t)rec[p] << 8 | (uint64_t)rec[p + 1] << 16 | (uint64_t)':' << 24, 4u);
        p += 3u;
        if (type == 'A') {
            if (p + 1u > len) return kSamBad;
            s.bytes((uint64_t)'A' | (uint64_t)':' << 8 | (uint64_t)rec[p] << 16, 3u);
            p += 1u;
        } else if (type == 'Z' || type == 'H') {
            uint64_t e = p;
            while (e < len && rec[e] != 0) ++e;
            if (e >= len) return kSamBad;                                     // no NUL inside the record
            if (e - p > 0xFFFFFFFFull) return kSamBad;
            s.bytes((uint64_t)type | (uint64_t)':' << 8, 2u);
            s.str(rec + p, (uint32_t)(e - p));
            p = e + 1u;
        } else if (type == 'B') {
            if (p + 5u > len) return kSamBad;
            const uint32_t sub = rec[p], count = rd32(rec + p + 1), size = scalar_size(sub);
            p += 5u;
            if (!size || (uint64_t)count * size > len - p) return kSamBad;
            s.bytes((uint64_t)'B' | (uint64_t)':' << 8 | (uint64_t)sub << 16 | (uint64_t)',' << 24, 4u);
            for (uint32_t k = 0; k < count; ++k) {
                if (k) s.bytes(',', 1u);
                put_scalar(s, sub, rec + p + (uint64_t)k * size);
            }
            p += (uint64_t)count * size;
        } else {
            const uint32_t size = scalar_size(type);
            if (!size || p + size > len) return kSamBad;
            s.bytes((uint64_t)(type == 'f' ? 'f' : 'i') | (uint64_t)':' << 8, 2u);
            put_scalar(s, type, rec + p);
            p += size;
        }
    }
    s.bytes('\n', 1u);
    return kSamOk;
}

// kSamOk and *length = the bytes of the line, or kSamBad
SBX_FMT_HD uint32_t sam_line_length(const uint8_t* rec, uint64_t len, const RefNames& refs, uint64_t* length) {
    LengthSink s;
    const uint32_t st = walk_record(rec, len, refs, s);
    *length = s.n;
    return st;
}

// Writes the line to out[0, length), `length` as sam_line_length gave it.  kSamOverrun when the walk wanted to write more or ended
// with fewer bytes (then what was written is a prefix of the line and no byte lies outside out[0, length)).
SBX_FMT_HD uint32_t sam_line_emit(const uint8_t* rec, uint64_t len, const RefNames& refs, uint8_t* out, uint64_t length) {
    LineSink s;
    s.init(out, length);
    const uint32_t st = walk_record(rec, len, refs, s);
    s.row.finish();
    if (st != kSamOk) return st;
    return s.over || s.used != length ? kSamOverrun : kSamOk;
}

}  // namespace samc
}  // namespace sbx
