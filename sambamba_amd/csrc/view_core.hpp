// view_core.hpp -- the arithmetic of `sambamba view`'s record selection (sambamba/view.d) that can be wrong: the overlap of a record
// with a region, the subsampling hash and its threshold, and the flag test of --num-filter.  These are `__host__ __device__` (K12,
// view.hip, calls them with the very statements the CPU test checks: tests/native/view_host.cpp).  The --num-filter parser and the
// text of -I are host code.
//
// Overlap (BamReadFilter.findNext, BioD bio/std/hts/bam/randomaccessmanager.d:397-460, for one region [start, end) of ref_id r):
//     ref_id == r  &&  pos < end  &&  (pos > start || pos + basesCovered > start)
// A record that covers no bases (unmapped but placed, or without CIGAR) is selected strictly inside the region and not at pos == start.
// The region "*" (bam.unmappedReads) holds the records with ref_id < 0.
// Subsampling (SubsampleFilter, sambamba/utils/common/filtering.d:340-371): 64-bit FNV-1a over the read name without its NUL, then the
// eight bytes of the seed, least significant first; the record passes iff the low 32 bits are below (uint64)(2^32 * fraction).
#pragma once
#include <cstddef>
#include <cstdint>

#include "sort_core.hpp"

namespace sbx {
namespace viewc {

constexpr uint32_t kUnmappedRegion = 0xFFFFFFFFu;        // sbx_region::ref_id of "*"
constexpr uint64_t kFnvOffset = 14695981039346656037ull, kFnvPrime = 1099511628211ull;

// covered = basesCovered() (0 for a record flagged unmapped); positions are signed as in the record
SBX_SORT_HD bool overlaps(int32_t ref_id, int32_t pos, uint32_t covered, uint32_t r_ref, uint32_t r_start, uint32_t r_end) {
    if (r_ref == kUnmappedRegion) return ref_id < 0;
    if (ref_id < 0 || (uint32_t)ref_id != r_ref) return false;
    const int64_t p = pos;
    return p < (int64_t)r_end && (p > (int64_t)r_start || p + (int64_t)covered > (int64_t)r_start);
}

SBX_SORT_HD uint64_t name_seed_hash(const uint8_t* name, uint32_t name_len, uint64_t seed) {
    uint64_t h = kFnvOffset;
    for (uint32_t k = 0; k < name_len; ++k) { h ^= name[k]; h *= kFnvPrime; }
    for (uint32_t k = 0; k < 8; ++k) { h ^= (seed >> (8 * k)) & 0xFFull; h *= kFnvPrime; }
    return h;
}

SBX_SORT_HD bool subsample_keeps(uint64_t hash, uint64_t threshold) { return (hash & 0xFFFFFFFFull) < threshold; }

SBX_SORT_HD bool flags_pass(uint32_t flag, uint32_t bits_set, uint32_t bits_unset) {
    return (flag & bits_set) == bits_set && (flag & bits_unset) == 0;
}

}  // namespace viewc
}  // namespace sbx

// ---- host only ----
#include <string>
#include <vector>

namespace sbx {
namespace viewc {

// (0x100000000UL * fraction).to!ulong: a double product, truncated.  false for a negative or NaN fraction (to!ulong throws), and for
// one whose product does not fit.
inline bool subsample_threshold(double fraction, uint64_t* threshold) {
    const double t = 4294967296.0 * fraction;
    if (!(t >= 0.0) || t >= 18446744073709551616.0) return false;
    *threshold = (uint64_t)t;
    return true;
}

// --num-filter=i1/i2 (view.d:271-277): split at '/', the first two pieces are unsigned 16-bit decimals (to!ushort), an empty piece
// is 0, further pieces are ignored.
inline bool parse_num_filter(const char* text, uint16_t* bits_set, uint16_t* bits_unset) {
    const std::string s = text ? text : "";
    std::vector<std::string> parts;
    if (!s.empty()) {                                         // (splitter of an empty string yields nothing)
        size_t p = 0;
        for (;;) {
            const size_t q = s.find('/', p);
            parts.push_back(s.substr(p, q == std::string::npos ? std::string::npos : q - p));
            if (q == std::string::npos) break;
            p = q + 1;
        }
    }
    uint16_t v[2] = {0, 0};
    for (size_t k = 0; k < 2 && k < parts.size(); ++k) {
        const std::string& t = parts[k];
        if (t.empty()) continue;
        uint32_t x = 0;
        for (char c : t) {
            if (c < '0' || c > '9') return false;
            x = x * 10 + (uint32_t)(c - '0');
            if (x > 0xFFFFu) return false;
        }
        v[k] = (uint16_t)x;
    }
    *bits_set = v[0];
    *bits_unset = v[1];
    return true;
}

// writeStringJson (BioD bio/core/utils/format.d:214-248): \b \t \n \f \r \" \\ -- and '?' written as \/ , because the table holds
// the solidus at index 63.  Every other byte is copied.
inline void json_string(const std::string& s, std::string* out) {
    out->push_back('"');
    for (char c : s) {
        char e = 0;
        switch (c) {
            case 8: e = 'b'; break;
            case 9: e = 't'; break;
            case 10: e = 'n'; break;
            case 12: e = 'f'; break;
            case 13: e = 'r'; break;
            case '"': e = '"'; break;
            case '?': e = '/'; break;
            case '\\': e = '\\'; break;
            default: break;
        }
        if (e) { out->push_back('\\'); out->push_back(e); }
        else out->push_back(c);
    }
    out->push_back('"');
}

// outputReferenceInfoJson (view.d:98-118) as its code prints it: the quote sits in front of the brace, `"{name":`.
inline std::string reference_info_json(const std::vector<std::string>& names, const std::vector<int64_t>& lengths) {
    std::string out = "[";
    for (size_t i = 0; i < names.size(); ++i) {
        if (i) out += ',';
        out += "\"{name\":";
        json_string(names[i], &out);
        out += ",\"length\":" + std::to_string(lengths[i]) + "}";
    }
    out += "]\n";
    return out;
}

}  // namespace viewc
}  // namespace sbx
