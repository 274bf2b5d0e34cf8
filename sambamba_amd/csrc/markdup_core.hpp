// markdup_core.hpp -- what `sambamba markdup` (sambamba/markdup.d) needs besides the kernels: the 5' coordinate and the score of a
// record, the hash that brings the two ends of a pair together, the keys whose unsigned order is the order of the reference's
// comparators, the end1 / end2 swap, and the header text of the output.  The record functions are `__host__ __device__` (K10,
// markdup.hip, uses the very statements the CPU test checks: tests/native/markdup_host.cpp); the header text is host code.
//
// Position key (singleEndInfoComparator, markdup.d:615-624: library, ref_id, coord, reversed -- all signed):
//     key = (library + 1) << (33 + ref_bits) | ref_id << 33 | (uint32)(coord ^ 0x80000000) << 1 | reversed
// library -1 (no RG, or one the header does not know) becomes 0 and sorts first; the coordinate is biased so that negative ones
// sort in front.  ref_bits is the width of the largest reference id of the file; a file whose libraries and references do not fit
// 30 bits together is refused by the caller (key_fits).
// Pair key (pairedEndsInfoComparator, markdup.d:626-641: library, ref1, coord1, reversed1, reversed2, ref2, coord2), three words,
// most significant first:  w0 = position key of end1;  w1 = reversed2 << 63 | ref2 << 32 | biased coord2;  w2 = ~score.
// Sorted by a STABLE sort from entries in file order of the earlier record, the first pair of a (w0, w1) group is the one with the
// highest score and, among equals, the one whose earlier record comes first in the file.
#pragma once
#include <cstddef>
#include <cstdint>

#include "sort_core.hpp"

namespace sbx {
namespace mdc {

constexpr uint32_t kCoordShift = 1, kRefShift = 33;
constexpr uint64_t kFragmentBit = 1ull << 32;        // single-end word: set for a fragment, clear for an unmatched paired read / a marker

SBX_SORT_HD uint32_t ld32u(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// computeFivePrimeCoord (markdup.d:699-708).  cigar: n_cigar little-endian words at any byte address.
SBX_SORT_HD int32_t five_prime_coord(int32_t pos, bool reversed, const uint8_t* cigar, uint32_t n_cigar) {
    if (!reversed) {
        uint32_t clip = 0;
        for (uint32_t k = 0; k < n_cigar; ++k) {
            const uint32_t c = ld32u(cigar + 4 * k), op = c & 15u;
            if (op != 4u && op != 5u) break;                 // S, H
            clip += c >> 4;
        }
        return (int32_t)((uint32_t)pos - clip);
    }
    uint32_t covered = 0, clip = 0;
    bool at_end = true;
    for (uint32_t k = n_cigar; k-- > 0;) {
        const uint32_t c = ld32u(cigar + 4 * k), op = c & 15u, len = c >> 4;
        if (at_end && (op == 4u || op == 5u)) { clip += len; continue; }
        at_end = false;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) covered += len;      // M D N = X
    }
    return (int32_t)((uint32_t)pos + covered + clip);
}

// computeScore (markdup.d:710-712): the sum of the base qualities that are at least 15
SBX_SORT_HD uint32_t score_of(const uint8_t* qual, uint32_t l_seq) {
    uint32_t s = 0;
    for (uint32_t k = 0; k < l_seq; ++k) s += qual[k] >= 15u ? qual[k] : 0u;
    return s;
}

// 64-bit FNV-1a over the read name, a zero byte and the RG string (readsArePaired compares exactly these); equal hashes are only a
// hint, K10b compares the bytes.
constexpr uint64_t kHashSeed = 14695981039346656037ull;
SBX_SORT_HD uint64_t hash_bytes(uint64_t h, const uint8_t* p, uint32_t n) {
    for (uint32_t k = 0; k < n; ++k) { h ^= p[k]; h *= 1099511628211ull; }
    return h;
}
SBX_SORT_HD uint64_t pair_hash(const uint8_t* name, uint32_t name_len, const uint8_t* rg, uint32_t rg_len) {
    uint64_t h = hash_bytes(kHashSeed, name, name_len);
    h ^= 0u; h *= 1099511628211ull;
    h = hash_bytes(h, rg, rg_len);
    return h ^ (h >> 29);
}

SBX_SORT_HD uint32_t ref_bits_of(int32_t n_ref) { return n_ref > 1 ? sortc::bit_width64((uint64_t)(n_ref - 1)) : 0; }
// do n_lib libraries (ids 0 .. n_lib - 1, and -1) and n_ref references fit the position key?
SBX_SORT_HD bool key_fits(int32_t n_lib, int32_t n_ref) { return kRefShift + ref_bits_of(n_ref) + sortc::bit_width64((uint64_t)n_lib) <= 63; }

SBX_SORT_HD uint64_t pos_key(int32_t library, int32_t ref_id, int32_t coord, uint32_t reversed, uint32_t ref_bits) {
    return (uint64_t)(uint32_t)(library + 1) << (kRefShift + ref_bits) | (uint64_t)(uint32_t)ref_id << kRefShift |
           (uint64_t)((uint32_t)coord ^ 0x80000000u) << kCoordShift | (reversed & 1u);
}

// combine (markdup.d:731-753): a is the earlier record in the file, b the later one; when b is strictly smaller on (ref_id, coord,
// reversed) the two are swapped (both carry the same library, so that is the order of their position keys).  w[0 .. 2]: the pair
// key; *end2: the position key of the second end, the marker the fragments at that place look for.
SBX_SORT_HD void pair_words(uint64_t key_a, uint32_t score_a, uint64_t key_b, uint32_t score_b, uint32_t ref_bits, uint64_t* w, uint64_t* end2) {
    const bool swap = key_b < key_a;
    const uint64_t k1 = swap ? key_b : key_a, k2 = swap ? key_a : key_b;
    const uint64_t ref2 = (k2 >> kRefShift) & ((1ull << ref_bits) - 1ull);
    w[0] = k1;
    w[1] = (k2 & 1ull) << 63 | ref2 << 32 | ((k2 >> kCoordShift) & 0xFFFFFFFFull);
    w[2] = (uint64_t)(uint32_t)~(score_a + score_b);
    *end2 = k2;
}

// second word of a single end: markers and unmatched paired reads (0) in front of the fragments, those by descending score
SBX_SORT_HD uint64_t single_word(bool fragment, uint32_t score) { return fragment ? kFragmentBit | (uint32_t)~score : 0ull; }

// ---- the flag rule (markdup.d:1286-1298), in one place: K10d, the streamed path's output plan and the CPU test use these ----
// the flag a record is written with: a marked record gets 0x400; an unmarked one loses it unless it is secondary or supplementary
SBX_SORT_HD uint32_t flag_after(uint32_t flag, bool dup) {
    if (dup) return flag | 0x400u;
    return (flag & 0x900u) ? flag : flag & ~0x400u;
}
// is a record with that resulting flag written?  (-r drops whatever carries 0x400, a secondary record that came with it included)
SBX_SORT_HD bool kept(uint32_t flag_after_, bool remove) { return !(remove && (flag_after_ & 0x400u)); }

// ---- the key store of the streamed path (K10e): what K10b compares of a pairable record, without the record ----
// An entry is  l_read_name (one byte) | the l_read_name bytes of the name | the RG:Z value | NUL  -- an absent RG is the NUL alone, so
// absent equals empty, as in the resident comparison.  The leading length byte makes two entries equal exactly when the resident
// comparison (same l_read_name, same name bytes, same RG string) says so -- also for a name that lacks its NUL or holds one inside,
// where name bytes and RG bytes could otherwise change places.  It also makes an entry self-describing: no array of lengths is kept.
// rec: the record from its block_size on; rg_at: offset of the RG:Z value in it (0: none); rg_len: its length without the NUL.
SBX_SORT_HD uint32_t pair_key_len(uint32_t l_name, uint32_t rg_len) { return 1u + l_name + rg_len + 1u; }
SBX_SORT_HD uint8_t pair_key_byte(const uint8_t* rec, uint32_t l_name, uint32_t rg_at, uint32_t rg_len, uint32_t k) {
    if (k == 0) return (uint8_t)l_name;
    if (k <= l_name) return rec[36u + k - 1u];
    const uint32_t j = k - 1u - l_name;
    return (rg_at && j < rg_len) ? rec[rg_at + j] : (uint8_t)0;
}
// two entries of the key store: same length and same bytes (the RG part ends at the entry's own NUL)
SBX_SORT_HD bool pair_keys_equal(const uint8_t* p, const uint8_t* q) {
    const uint32_t ln = p[0];
    if (ln != q[0]) return false;
    for (uint32_t k = 1; k <= ln; ++k) if (p[k] != q[k]) return false;
    for (uint32_t k = ln + 1u;; ++k) {
        if (p[k] != q[k]) return false;
        if (!p[k]) return true;
    }
}

}  // namespace mdc
}  // namespace sbx

// ---- host only ----
namespace sbx {
namespace mdc {

// ReadGroupIndex (markdup.d:659-696): per @RG line of the parsed header the index of first appearance of its LB string (an absent LB
// is the empty string, a library like any other); returns the number of libraries.
inline int32_t read_group_libraries(const sortc::ParsedHeader& h, std::vector<int32_t>* library_of) {
    std::vector<std::string> libs;
    library_of->clear();
    for (const std::string& lb : h.rg_library) {
        size_t k = 0;
        while (k < libs.size() && libs[k] != lb) ++k;
        if (k == libs.size()) libs.push_back(lb);
        library_of->push_back((int32_t)k);
    }
    return (int32_t)libs.size();
}

// The header `sambamba markdup` writes: toSam of the parsed input -- SO only when the first line is an @HD that names one of
// unsorted / coordinate / queryname (header.d:488-499, 626-633) -- after addPG (utils/version_.d:9-22) put
// "@PG ID:sambamba CL:<command_line> PP:<ID of the last @PG> VN:1.0" behind the programs; a header that has an @PG with ID:sambamba
// keeps it instead (the dictionary refuses the second one).  command_line == nullptr: no @PG is added.
inline bool markdup_header_text(const char* text, size_t n, const char* command_line, std::string* out, std::string* why) {
    sortc::ParsedHeader h;
    if (!sortc::parse_header(text, n, &h, why)) return false;
    const std::string& so = h.sorting_order;
    const bool known = so == "unsorted" || so == "coordinate" || so == "queryname";
    if (command_line) {
        bool have = false;
        for (const sortc::HeaderLine& l : h.pg) have = have || l.id == "sambamba";
        if (!have) {
            sortc::HeaderLine l;
            l.id = "sambamba";
            l.text = "@PG\tID:sambamba";
            if (*command_line) l.text += std::string("\tCL:") + command_line;
            if (!h.pg.empty() && !h.pg.back().id.empty()) l.text += "\tPP:" + h.pg.back().id;
            l.text += "\tVN:1.0";
            h.pg.push_back(l);
        }
    }
    *out = sortc::serialise_header(h, known ? so : std::string());
    return true;
}

}  // namespace mdc
}  // namespace sbx
