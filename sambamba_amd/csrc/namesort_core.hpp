// namesort_core.hpp -- what `sambamba sort -n / -N / -M` needs besides the kernels: the two read-name comparators as the reference
// states them, the encoder that turns a name into a byte string whose plain unsigned order IS the comparator's order, and the -M
// word (HI tag, flag).  `__host__ __device__`: K14 (namesort.hip) runs the very statements the CPU test checks
// (tests/native/namesort_host.cpp), and tools/sort_cpu sorts with the comparators.
//
// Orders (BioD bio/std/hts/bam/read.d:1493-1621, applied by a stable merge sort):
//   -n  compareReadNames: a.name < b.name on D strings -- byte-wise, unsigned, a proper prefix first.
//   -N  mixedStrCompare(a.name, b.name) < 0: bytes compare as bytes, but where both strings stand at a digit the two digit runs
//       compare as numbers (leading zeros skipped; more significant digits is greater; then the first differing digit), and runs of
//       equal value compare by their number of leading zeros.  When one string ends, the shorter is less.
//   -M  among equal names: ascending HI tag (absent: 0), then ascending flag.
//
// The key of a name: bytes, all non-zero, packed big-endian into 64-bit words, the last word padded with zero bytes -- so "the key
// ends here" sorts below every continuation, and the order of two keys is the order of their words taken as unsigned numbers,
// a missing word counting as 0.
//   -n  the name bytes themselves.
//   -N  a byte that is no digit: itself.  A digit run with nz leading zeros and nsig digits behind them:
//           '0', nsig + 1, the nsig digits, nz + 1
//       The class byte '0' orders against a byte that is no digit as any digit would (no such byte lies in '0'..'9'); nsig before
//       the digits makes the longer number the greater one; nz comes behind the digits, where the comparator looks at it.  A name
//       has at most 254 bytes, so nsig + 1 and nz + 1 fit a byte; the key has at most 635 bytes (digit, non-digit, digit, ...).
// Names are restricted to bytes 0x01..0x7F (name_ok): there the reference's signed (-N) and unsigned (-n) byte orders agree.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SBX_NS_HD __host__ __device__ __forceinline__
#else
#define SBX_NS_HD inline
#endif

namespace sbx {
namespace nsc {

enum : uint32_t { kOrderLex = 1, kOrderNatural = 2 };          // the `order` argument of sbx_sort_bam_by_name
constexpr uint32_t kMaxNameLen = 254;                            // l_read_name is one byte and counts the NUL
constexpr uint32_t kMaxKeyWords = 80;                            // 635 key bytes at most

SBX_NS_HD bool is_digit(uint8_t c) { return c >= '0' && c <= '9'; }

// ---- the comparators, as the specification states them ----
SBX_NS_HD bool name_less(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    const uint32_t m = na < nb ? na : nb;
    for (uint32_t k = 0; k < m; ++k)
        if (a[k] != b[k]) return a[k] < b[k];
    return na < nb;
}

SBX_NS_HD int mixed_str_compare(const uint8_t* a, uint32_t na, const uint8_t* b, uint32_t nb) {
    uint32_t i = 0, j = 0;                                       // the fronts
    while (i < na && j < nb) {
        if (is_digit(a[i]) && is_digit(b[j])) {
            int za = 0, zb = 0;
            while (i < na && a[i] == '0') { ++za; ++i; }
            while (j < nb && b[j] == '0') { ++zb; ++j; }
            while (i < na && j < nb && is_digit(a[i]) && a[i] == b[j]) { ++i; ++j; }
            const bool da = i < na && is_digit(a[i]), db = j < nb && is_digit(b[j]);
            if (da && db) {
                uint32_t k = 0;
                const uint32_t ra = na - i, rb = nb - j, maxk = ra < rb ? ra : rb;
                while (k < maxk && is_digit(a[i + k]) && is_digit(b[j + k])) ++k;
                if (k < ra && is_digit(a[i + k])) return 1;      // a has more digits
                if (k < rb && is_digit(b[j + k])) return -1;
                return (int)(int8_t)a[i] - (int)(int8_t)b[j];
            }
            if (da) return 1;
            if (db) return -1;
            if (za != zb) return za - zb;
        } else {
            if (a[i] != b[j]) return (int)(int8_t)a[i] - (int)(int8_t)b[j];
            ++i; ++j;
        }
    }
    return i < na ? 1 : j < nb ? -1 : 0;
}

// every byte in 0x01..0x7F
SBX_NS_HD bool name_ok(const uint8_t* name, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k)
        if (name[k] == 0 || name[k] > 0x7F) return false;
    return true;
}

// ---- the key: ONE walker hands the key bytes to a sink; LengthSink adds them up, WordSink writes them ----
template <class Sink>
SBX_NS_HD void walk_key(const uint8_t* name, uint32_t n, uint32_t order, Sink& sink) {
    if (order != kOrderNatural) {
        for (uint32_t k = 0; k < n; ++k) sink.put(name[k]);
        return;
    }
    uint32_t k = 0;
    while (k < n) {
        if (!is_digit(name[k])) { sink.put(name[k++]); continue; }
        const uint32_t z0 = k;
        while (k < n && name[k] == '0') ++k;
        const uint32_t s0 = k;
        while (k < n && is_digit(name[k])) ++k;
        sink.put('0');
        sink.put((uint8_t)(k - s0 + 1));
        for (uint32_t d = s0; d < k; ++d) sink.put(name[d]);
        sink.put((uint8_t)(s0 - z0 + 1));
    }
}

struct LengthSink {
    uint32_t n = 0;
    SBX_NS_HD void put(uint8_t) { ++n; }
};

// big-endian into out[0, cap): a word is stored once, when it is full or at finish(); a byte behind word cap - 1 is dropped
struct WordSink {
    uint64_t* out;
    uint32_t cap;
    uint64_t cur = 0;
    uint32_t n = 0;                                              // bytes taken
    bool overrun = false;
    SBX_NS_HD WordSink(uint64_t* o, uint32_t c) : out(o), cap(c) {}
    SBX_NS_HD void put(uint8_t b) {
        const uint32_t w = n >> 3;
        if (w >= cap) { overrun = true; return; }
        cur |= (uint64_t)b << (56u - 8u * (n & 7u));
        ++n;
        if (!(n & 7u)) { out[w] = cur; cur = 0; }
    }
    SBX_NS_HD void finish() {
        if (n & 7u) out[n >> 3] = cur;                           // (n >> 3 < cap: put() admitted the byte)
    }
};

SBX_NS_HD uint32_t key_bytes(const uint8_t* name, uint32_t n, uint32_t order) {
    LengthSink s;
    walk_key(name, n, order, s);
    return s.n;
}
SBX_NS_HD uint32_t key_words(const uint8_t* name, uint32_t n, uint32_t order) { return (key_bytes(name, n, order) + 7u) / 8u; }
// writes the key into out[0, cap) and returns the words it has; false when it has more than cap (nothing behind out + cap is written)
SBX_NS_HD bool key_emit(const uint8_t* name, uint32_t n, uint32_t order, uint64_t* out, uint32_t cap, uint32_t* words) {
    WordSink s(out, cap);
    walk_key(name, n, order, s);
    s.finish();
    *words = (s.n + 7u) / 8u;
    return !s.overrun;
}

// ---- -M ----
SBX_NS_HD uint32_t ld16(const uint8_t* p) { uint16_t v; __builtin_memcpy(&v, p, 2); return v; }
SBX_NS_HD uint32_t ld32(const uint8_t* p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }

// The value of the first HI tag among the aux fields rec[t, e) (getHI, read.d:1583-1592): *hi = 0 when there is none.  false: the
// tag is of no integer type (c C s S i I) or does not fit an int (the reference throws), or a tag in front of it is of unknown type
// or runs past e.  No byte at or behind rec + e is read.
SBX_NS_HD bool find_hi(const uint8_t* rec, uint64_t t, uint64_t e, int32_t* hi) {
    *hi = 0;
    while (t < e) {
        if (t + 3 > e) return false;
        const uint8_t k0 = rec[t], k1 = rec[t + 1], ty = rec[t + 2];
        t += 3;
        const bool is_hi = k0 == 'H' && k1 == 'I';
        uint64_t size;
        switch (ty) {
            case 'A': case 'c': case 'C': size = 1; break;
            case 's': case 'S': size = 2; break;
            case 'i': case 'I': case 'f': size = 4; break;
            case 'Z': case 'H': {
                if (is_hi) return false;
                uint64_t z = t;
                while (z < e && rec[z]) ++z;
                if (z >= e) return false;                        // not terminated inside the record
                size = z + 1 - t;
                break;
            }
            case 'B': {
                if (is_hi || t + 5 > e) return false;
                const uint8_t sub = rec[t];
                const uint64_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
                if (!w) return false;
                size = 5 + (uint64_t)ld32(rec + t + 1) * w;
                break;
            }
            default: return false;
        }
        if (size > e - t) return false;
        if (is_hi) {
            switch (ty) {
                case 'c': *hi = (int8_t)rec[t]; return true;
                case 'C': *hi = rec[t]; return true;
                case 's': *hi = (int16_t)ld16(rec + t); return true;
                case 'S': *hi = (int32_t)ld16(rec + t); return true;
                case 'i': *hi = (int32_t)ld32(rec + t); return true;
                case 'I': { const uint32_t v = ld32(rec + t); *hi = (int32_t)v; return v <= 0x7FFFFFFFu; }
                default: return false;                           // A, f
            }
        }
        t += size;
    }
    return true;
}

// the word that orders equal names under -M: HI as a signed number, then the flag
SBX_NS_HD uint64_t mate_word(int32_t hi, uint32_t flag) { return (uint64_t)((uint32_t)hi ^ 0x80000000u) << 16 | (flag & 0xFFFFu); }

// Where the name and the aux fields of a record of `len` bytes (block_size included) lie; false when its lengths contradict len.
struct NameFrame { uint32_t name_len; uint32_t flag; uint64_t aux; bool aux_ok; };
SBX_NS_HD bool name_frame(const uint8_t* rec, uint64_t len, NameFrame* f) {
    if (len < 36) return false;
    const uint32_t l_name = rec[12];
    if (l_name < 1 || 36ull + l_name > len || rec[36 + l_name - 1] != 0) return false;
    f->name_len = l_name - 1;
    const uint32_t fnc = ld32(rec + 16);
    f->flag = fnc >> 16;
    const int32_t l_seq = (int32_t)ld32(rec + 20);
    const uint64_t seq = l_seq < 0 ? 0 : (uint64_t)l_seq;
    f->aux = 36ull + l_name + 4ull * (fnc & 0xFFFFu) + (seq + 1) / 2 + seq;
    f->aux_ok = l_seq >= 0 && f->aux <= len;
    return true;
}

}  // namespace nsc
}  // namespace sbx
