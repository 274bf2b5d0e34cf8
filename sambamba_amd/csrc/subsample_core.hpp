// subsample_core.hpp -- the arithmetic of `sbx-subsample` (K22, subsample.hip; engine_subsample.cpp) that can be wrong: which records
// count towards the coverage, the span a counted record covers with its clips, the slot arithmetic of the coverage array, and the
// predicate that keeps or drops a record.  `__host__ __device__`: K22a and K22c run the very statements tests/native/subsample_host.cpp
// checks on the CPU.  The definition is DESIGN.md section 8, "subsample"; the reference's subsample.d is unfinished (it never drops a
// read), its header comment and usage text are what this follows.
//
//   counted   flag has none of 0x4 (unmapped), 0x200 (QC fail), 0x400 (duplicate); 0 <= ref_id < n_ref; 0 <= pos < LN[ref_id]
//   span      [pos, e), e = min(pos + max(basesCovered, 1), LN); basesCovered as binc::expected_bin adds it up (M D N = X, 32 bits)
//   slots     reference r owns slots [base[r], base[r + 1]) of the coverage array D, base[r] = sum over q < r of (LN[q] + 1): one
//             slot per position and one more, which takes the -1 of a span that ends at LN.  A counted record adds +1 at
//             base[r] + pos and -1 (0xFFFFFFFF) at base[r] + e; both lie inside r's slots, every reference's marks add up to 0, so
//             ONE inclusive scan over the concatenation turns D into the coverage c_r(p) at base[r] + p, modulo 2^32 exactly.
//   verdict   cov = max(c(pos), c(e - 1)); h = low 32 bits of viewc::name_seed_hash(name, 0); kept iff cov <= max_cov or
//             (uint64) h * cov < (uint64) max_cov << 32
#pragma once
#include <cstddef>
#include <cstdint>

#include "sort_core.hpp"

namespace sbx {
namespace subc {

constexpr uint32_t kCovTile = 4096;             // words of D per workgroup of the scan (K22b)
constexpr uint32_t kUncountedFlags = 0x4u | 0x200u | 0x400u;
constexpr uint32_t kDroppedFlag = 0x200u;       // what a dropped record is marked with when it is not removed

SBX_SORT_HD uint32_t load32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// ln: LN of the record's reference (not read unless 0 <= ref_id < n_ref)
SBX_SORT_HD bool counted(uint32_t flag, int32_t ref_id, int32_t n_ref, int32_t pos, int64_t ln) {
    return !(flag & kUncountedFlags) && ref_id >= 0 && ref_id < n_ref && pos >= 0 && (int64_t)pos < ln;
}

// e of a counted record (0 <= pos < ln): pos + max(bases, 1) in 64 bits, so a sum that passes 2^31 is clipped by ln
SBX_SORT_HD uint32_t span_end(int32_t pos, uint32_t bases, int64_t ln) {
    const uint64_t e = (uint64_t)(uint32_t)pos + (bases ? bases : 1u);
    return (uint32_t)(e < (uint64_t)ln ? e : (uint64_t)ln);
}

SBX_SORT_HD bool keeps(uint32_t h, uint32_t cov, uint32_t max_cov) {
    return cov <= max_cov || (uint64_t)h * cov < ((uint64_t)max_cov << 32);
}

// slots of a reference of length ln (a negative length counts as 0), and of D rounded up to whole tiles of the scan
SBX_SORT_HD uint64_t ref_slots(int64_t ln) { return (uint64_t)(ln > 0 ? ln : 0) + 1; }
SBX_SORT_HD uint64_t cov_tiles(uint64_t slots) { return (slots + kCovTile - 1) / kCovTile; }
// LN of reference r from the slot bases (base has n_ref + 1 entries)
SBX_SORT_HD int64_t ref_length(const uint64_t* base, int32_t r) { return (int64_t)(base[r + 1] - base[r]) - 1; }

struct Span {
    bool counted;
    uint32_t flag, bs;
    uint64_t lo, hi;            // counted: slots of pos and of e in D; hi - 1 is the slot of the span's last position
    uint32_t name_len;          // bytes of the name without its NUL
};
// rec: the record from its block_size field on, bs = that field; the caller has checked that 4 + bs bytes are readable and
// bs >= 32.  false: the name and the CIGAR the record states run past its block_size (nothing behind the fixed part is read then).
SBX_SORT_HD bool record_span(const uint8_t* rec, uint32_t bs, const uint64_t* base, int32_t n_ref, Span* s) {
    const int32_t ref_id = (int32_t)load32(rec + 4), pos = (int32_t)load32(rec + 8);
    const uint32_t l_name = rec[12], fnc = load32(rec + 16);
    const uint32_t n_cigar = fnc & 0xFFFFu;
    if (32ull + l_name + 4ull * n_cigar > bs) return false;
    s->flag = fnc >> 16;
    s->bs = bs;
    s->name_len = l_name ? l_name - 1 : 0;
    s->lo = s->hi = 0;
    const int64_t ln = ref_id >= 0 && ref_id < n_ref ? ref_length(base, ref_id) : 0;
    s->counted = counted(s->flag, ref_id, n_ref, pos, ln);
    if (!s->counted) return true;
    uint32_t bases = 0;
    const uint8_t* cg = rec + 36 + l_name;
    for (uint32_t k = 0; k < n_cigar; ++k) {
        const uint32_t op = load32(cg + 4u * k), ty = op & 15u;
        if (ty == 0u || ty == 2u || ty == 3u || ty == 7u || ty == 8u) bases += op >> 4;
    }
    s->lo = base[ref_id] + (uint32_t)pos;
    s->hi = base[ref_id] + span_end(pos, bases, ln);
    return true;
}

}  // namespace subc
}  // namespace sbx

// ---- host only ----
#include <vector>

namespace sbx {
namespace subc {

// base[0 .. n_ref]: where every reference's slots start in D; base[n_ref] is the number of slots
inline std::vector<uint64_t> slot_bases(const int32_t* ln, size_t n_ref) {
    std::vector<uint64_t> base(n_ref + 1, 0);
    for (size_t r = 0; r < n_ref; ++r) base[r + 1] = base[r] + ref_slots(ln[r]);
    return base;
}

}  // namespace subc
}  // namespace sbx
