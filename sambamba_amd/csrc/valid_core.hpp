// valid_core.hpp -- is a BAM record valid?  isValid / BooleanValidator of BioD bio/std/hts/bam/validation/alignment.d, with the parts of
// bam/read.d (name, cigar, base_qualities, opApply over the tags: 1173-1186) and bam/tagvalue.d (readValueFromArray: 541-588) it calls,
// restated `__host__ __device__`: K19 (valid.hip) runs it per record, tests/native/valid_host.cpp runs it on the CPU under the
// sanitizers.  Under the BooleanValidator every onError returns false, so the first error of any kind makes the record invalid; the
// mask returned here does not stop there -- every class is evaluated on its own -- and a record is valid iff it is 0.
//
// ONE walker, next_tag, goes through the tags; the value rules (tag_ok) and the duplicate search (key_seen_before) both sit on it.
//   * reads: nothing at or behind rec + avail is read.  The fixed part is checked as a whole (36 bytes, block_size against avail,
//     then name, CIGAR, sequence and qualities against block_size); next_tag checks every tag against the end of the record before a
//     byte of its value is read.
//   * kMalformed is this project's: on such records the reference reads past the record or throws.  When the fixed part is malformed
//     nothing else is evaluated and the mask is kMalformed alone; when a tag is, the classes in front of the tags are evaluated,
//     kTagValue / kTagDuplicate cover the tags in front of the break, and kMalformed is added.
//   * the tag loop of the reference runs `while (offset + 1 < length)`: ONE byte left over behind the last tag is not looked at and
//     is no error; two or more start a tag.
//   * qualities: eight bytes per load, the rest one by one (never a load that passes the last quality).
#pragma once
#include "format_core.hpp"

namespace sbx {
namespace validc {

// bit k of the mask = class k of the report (sbx_validate_report::class_count[k])
enum : uint16_t {
    kNameEmpty = 1u << 0,       // EmptyReadName
    kNameChars = 1u << 1,       // ReadNameContainsInvalidCharacters.  (TooLongReadName cannot occur: l_read_name is one byte, so a name
                                // without its NUL has at most 254 bytes)
    kPosition = 1u << 2,        // PositionIsOutOfRange
    kQualities = 1u << 3,       // QualityDataContainsInvalidElements
    kCigarHard = 1u << 4,       // InternalHardClipping
    kCigarSoft = 1u << 5,       // InternalSoftClipping
    kCigarLength = 1u << 6,     // InconsistentLength
    kTagValue = 1u << 7,        // InvalidTags
    kTagDuplicate = 1u << 8,    // DuplicateTagKeys
    kMalformed = 1u << 9,
};
constexpr int kClasses = 10;

SBX_FMT_HD uint32_t rd16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
SBX_FMT_HD uint32_t rd32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
SBX_FMT_HD uint64_t rd64(const uint8_t* p) { uint64_t v; __builtin_memcpy(&v, p, 8); return v; }

SBX_FMT_HD bool is_digit(uint32_t c) { return c - '0' < 10u; }
SBX_FMT_HD bool is_upper(uint32_t c) { return c - 'A' < 26u; }
SBX_FMT_HD bool is_hex(uint32_t c) { return is_digit(c) || (c | 0x20u) - 'a' < 6u; }
SBX_FMT_HD bool is_graph(uint32_t c) { return c - '!' <= (uint32_t)('~' - '!'); }       // [!-~]

// bytes of a value of primitive type t / of an element of a B array; 0: no such type (UnknownTagTypeException)
SBX_FMT_HD uint32_t elem_size(uint32_t t) {
    switch (t) {
        case 'c': case 'C': return 1;
        case 's': case 'S': return 2;
        case 'i': case 'I': case 'f': return 4;
        default: return 0;
    }
}
SBX_FMT_HD uint32_t prim_size(uint32_t t) { return t == 'A' ? 1u : elem_size(t); }

// ---- the walker ----
struct Tag {
    uint32_t key;       // the two key bytes, first one low
    uint32_t type, sub; // type byte; element type of a B array
    uint32_t val;       // offset of the value (Z / H: the text; B: the first element) in the tag bytes
    uint32_t len;       // Z / H: bytes without the NUL; B: elements; else the size of the value
    uint32_t next;      // offset of the next tag
};
enum : uint32_t { kTagEnd = 0, kTagOk = 1, kTagBroken = 2 };

// the tag at offset off of the tl tag bytes t
SBX_FMT_HD uint32_t next_tag(const uint8_t* t, uint32_t tl, uint32_t off, Tag* g) {
    if (off + 1u >= tl) return kTagEnd;
    if (off + 3u > tl) return kTagBroken;                 // a key without a type
    g->key = rd16(t + off);
    g->type = t[off + 2];
    g->sub = 0;
    const uint32_t v = off + 3u;
    g->val = v;
    if (g->type == 'Z' || g->type == 'H') {
        uint32_t e = v;
        while (e < tl && t[e]) ++e;
        if (e >= tl) return kTagBroken;                   // no NUL
        g->len = e - v;
        g->next = e + 1u;
        return kTagOk;
    }
    if (g->type == 'B') {
        if (tl - v < 5u) return kTagBroken;
        g->sub = t[v];
        const uint32_t es = elem_size(g->sub);
        if (!es) return kTagBroken;
        const uint32_t n = rd32(t + v + 1);
        if ((uint64_t)n * es > (uint64_t)(tl - v - 5u)) return kTagBroken;
        g->val = v + 5u;
        g->len = n;
        g->next = v + 5u + n * es;
        return kTagOk;
    }
    const uint32_t ps = prim_size(g->type);
    if (!ps || tl - v < ps) return kTagBroken;
    g->len = ps;
    g->next = v + ps;
    return kTagOk;
}

// ---- the rules of one tag (isValid(key, value, al) and checkTagValue) ----
constexpr uint32_t key_of(char a, char b) { return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8; }
enum : uint32_t { kAnyType = 0, kWantInt = 1, kWantString = 2, kWantU16Array = 3 };

// PredefinedTags of alignment.d:83-119
SBX_FMT_HD uint32_t predefined(uint32_t key) {
    switch (key) {
        case key_of('A', 'M'): case key_of('A', 'S'): case key_of('C', 'M'): case key_of('C', 'P'): case key_of('F', 'I'):
        case key_of('H', '0'): case key_of('H', '1'): case key_of('H', '2'): case key_of('H', 'I'): case key_of('I', 'H'):
        case key_of('M', 'Q'): case key_of('N', 'H'): case key_of('N', 'M'): case key_of('O', 'P'): case key_of('P', 'Q'):
        case key_of('S', 'M'): case key_of('T', 'C'): case key_of('U', 'Q'):
            return kWantInt;
        case key_of('B', 'C'): case key_of('B', 'Q'): case key_of('C', 'C'): case key_of('C', 'Q'): case key_of('C', 'S'):
        case key_of('E', '2'): case key_of('F', 'S'): case key_of('L', 'B'): case key_of('M', 'D'): case key_of('O', 'Q'):
        case key_of('O', 'C'): case key_of('P', 'G'): case key_of('P', 'U'): case key_of('Q', '2'): case key_of('R', '2'):
        case key_of('R', 'G'): case key_of('U', '2'):
            return kWantString;
        case key_of('F', 'Z'):
            return kWantU16Array;
        default:
            return kAnyType;
    }
}

// ^[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*$ as alignment.d:487-520 spells it out; n >= 1
SBX_FMT_HD bool md_ok(const uint8_t* s, uint32_t n) {
    if (!is_digit(s[0])) return false;
    uint32_t i = 1;
    while (i < n && is_digit(s[i])) ++i;
    while (i < n) {
        if (is_upper(s[i])) ++i;
        else if (s[i] == '^') {
            ++i;
            if (i == n || !is_upper(s[i])) return false;
            while (i < n && is_upper(s[i])) ++i;
        } else return false;
        if (i == n || !is_digit(s[i])) return false;
        while (i < n && is_digit(s[i])) ++i;
    }
    return true;
}

// false: the tag breaks a rule.  Under the BooleanValidator the first broken rule ends the checks of the tag (`return false`), so the
// casts behind a type mismatch are never reached -- and never made here.
SBX_FMT_HD bool tag_ok(const uint8_t* t, const Tag& g, uint32_t l_seq) {
    const uint8_t* v = t + g.val;
    if (g.type == 'H') {
        if (!g.len) return false;                                          // EmptyHexadecimalString
        for (uint32_t k = 0; k < g.len; ++k)
            if (!is_hex(v[k])) return false;                               // InvalidHexadecimalString (an odd length is not looked at)
    } else if (g.type == 'A') {
        if (!is_graph(v[0])) return false;                                 // NonPrintableCharacter
    } else if (g.type == 'Z') {
        if (!g.len) return false;                                          // EmptyString
        for (uint32_t k = 0; k < g.len; ++k)
            if (v[k] < ' ' || v[k] > '~') return false;                    // NonPrintableString
    }
    const uint32_t want = predefined(g.key);
    if (want == kAnyType) return true;
    if (want == kWantInt) return g.type != 'A' && g.type != 'f' && elem_size(g.type) != 0;      // c C s S i I
    if (want == kWantU16Array) return g.type == 'B' && g.sub == 'S';
    if (g.type != 'Z') return false;                                       // ExpectedStringValue: also for H
    const uint32_t key = g.key;
    if (key == key_of('C', 'Q') || key == key_of('E', '2') || key == key_of('O', 'Q') || key == key_of('Q', '2') || key == key_of('U', '2')) {
        if (!(g.len == 1 && v[0] == '*'))
            for (uint32_t k = 0; k < g.len; ++k)
                if (!is_graph(v[k])) return false;                         // InvalidQualityString
    }
    if ((key == key_of('B', 'Q') || key == key_of('E', '2')) && g.len != l_seq) return false;
    if (key == key_of('M', 'D') && !md_ok(v, g.len)) return false;
    return true;
}

// does a tag in front of offset `at` carry `key`?  (the tags in front of `at` have been walked once: all are kTagOk)
SBX_FMT_HD bool key_seen_before(const uint8_t* t, uint32_t tl, uint32_t at, uint32_t key) {
    Tag g;
    for (uint32_t off = 0; off < at; off = g.next) {
        if (next_tag(t, tl, off, &g) != kTagOk) return false;
        if (g.key == key) return true;
    }
    return false;
}

// ---- the qualities: neither all 0xFF nor all <= 93 ----
SBX_FMT_HD bool qualities_bad(const uint8_t* q, uint32_t n) {
    uint64_t all = ~0ull, high = 0;           // AND of the bytes; bit 7 of a byte set where one was > 93
    uint32_t k = 0;
    for (; k + 8u <= n; k += 8u) {
        const uint64_t x = rd64(q + k);
        all &= x;
        high |= ((x & 0x7F7F7F7F7F7F7F7Full) + 0x2222222222222222ull) | x;      // (b & 127) + 34 >= 128 iff (b & 127) >= 94
    }
    for (; k < n; ++k) {
        const uint64_t b = q[k];
        all &= b | ~0xFFull;
        high |= b > 93u ? 0x80u : 0u;
    }
    return all != ~0ull && (high & 0x8080808080808080ull) != 0;
}

// ---- the record ----
// rec: the record from its block_size field on; avail: the bytes that may be read from rec on.
SBX_FMT_HD uint16_t record_mask(const uint8_t* rec, uint64_t avail) {
    if (avail < 36u) return kMalformed;
    const uint32_t bs = rd32(rec);
    if (bs < 32u || bs > 0x7FFFFFF0u || 4ull + bs > avail) return kMalformed;
    const int32_t pos = (int32_t)rd32(rec + 8);
    const uint32_t l_name = rec[12], n_cigar = rd32(rec + 16) & 0xFFFFu, l_seq = rd32(rec + 20);
    const uint64_t fixed = 32ull + l_name + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u + l_seq;
    if (l_name == 0 || fixed > bs) return kMalformed;        // (a negative l_seq is a huge one here)
    uint32_t m = 0;

    // invalidReadName: the name is the l_read_name - 1 bytes in front of the NUL (read.d name())
    const uint8_t* name = rec + 36;
    if (l_name == 1u) m |= kNameEmpty;
    for (uint32_t k = 0; k + 1u < l_name; ++k) {
        const uint32_t c = name[k];
        if (c < '!' || c > '~' || c == '@') { m |= kNameChars; break; }
    }
    // invalidPosition: [-1, 2^29 - 2]
    if (pos < -1 || pos > (1 << 29) - 2) m |= kPosition;
    // invalidCigar: nothing for an empty one
    const uint8_t* cg = name + l_name;
    if (n_cigar) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t op = rd32(cg + 4u * k), ty = op & 15u;          // "MIDNSHP=X????????"[ty]
            if (ty == 0u || ty == 1u || ty == 4u || ty == 7u || ty == 8u) sum += op >> 4;      // M I S = X, in 32 bits
            if (ty == 5u && n_cigar > 2u && k > 0u && k + 1u < n_cigar) m |= kCigarHard;
        }
        if ((int32_t)l_seq > 0 && l_seq != sum) m |= kCigarLength;
        if (n_cigar > 2u) {
            // one H off the front, then one off the back of what is left; S strictly inside the rest
            uint32_t lo = 0, hi = n_cigar;
            if ((rd32(cg) & 15u) == 5u) lo = 1;
            if ((rd32(cg + 4u * (hi - 1u)) & 15u) == 5u) --hi;
            if (hi - lo > 2u)
                for (uint32_t k = lo + 1u; k + 1u < hi; ++k)
                    if ((rd32(cg + 4u * k) & 15u) == 4u) { m |= kCigarSoft; break; }
        }
    }
    // invalidQualityData
    const uint8_t* qual = cg + 4ull * n_cigar + ((uint64_t)l_seq + 1u) / 2u;
    if (qualities_bad(qual, l_seq)) m |= kQualities;
    // invalidTags
    const uint8_t* t = rec + 4 + fixed;
    const uint32_t tl = (uint32_t)(bs - fixed);
    Tag g;
    for (uint32_t off = 0;; off = g.next) {
        const uint32_t st = next_tag(t, tl, off, &g);
        if (st == kTagEnd) break;
        if (st == kTagBroken) { m |= kMalformed; break; }
        if (!tag_ok(t, g, l_seq)) m |= kTagValue;
        if (!(m & kTagDuplicate) && key_seen_before(t, tl, off, g.key)) m |= kTagDuplicate;
    }
    return (uint16_t)m;
}

}  // namespace validc
}  // namespace sbx
