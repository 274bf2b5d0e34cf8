// slice_core.hpp -- the arithmetic of `sambamba slice` (sambamba/slice.d, the header comment) that can be wrong: which records lie in
// R1 of a region, where the copied stretch [a, b) of the inflated stream starts and ends, and how [a, b) falls into a head that is
// compressed again, a run of BGZF blocks that is copied from the file as it is, and a tail.  `__host__ __device__`: K18 (slice.hip)
// calls the predicates with the very statements the CPU test checks (tests/native/slice_host.cpp).
//
// For a region (r, beg, end) over the records i = 0 .. n-1 of a coordinate-sorted file:
//     R1          ref == r && pos < beg && pos + basesCovered > beg        (the reads that start in front of the region and reach it)
//     first_ge(x) the first record with ref < 0 || ref > r || (ref == r && pos >= x), else n
//     a, b        the stream offsets of first_ge(beg) and first_ge(end)
// R1 is written over viewc::overlaps (view_core.hpp) with the region [beg, beg + 1): one overlap predicate for view and slice.
#pragma once
#include <cstddef>
#include <cstdint>

#include "view_core.hpp"

namespace sbx {
namespace slicec {

// covered = basesCovered() (0 for a record flagged unmapped or without CIGAR): such a record is never in R1
SBX_SORT_HD bool in_r1(int32_t ref_id, int32_t pos, uint32_t covered, uint32_t r_ref, uint32_t beg) {
    return (int64_t)pos < (int64_t)beg && viewc::overlaps(ref_id, pos, covered, r_ref, beg, beg + 1u);
}

// the predicate of first_ge(x): true from some record of a sorted file on
SBX_SORT_HD bool at_or_behind(int32_t ref_id, int32_t pos, uint32_t r_ref, uint32_t x) {
    if (ref_id < 0 || (uint32_t)ref_id > r_ref) return true;
    return (uint32_t)ref_id == r_ref && (int64_t)pos >= (int64_t)x;
}

// [a, b) of the inflated stream over the block table out_off[0 .. n_blocks] (out_off[n_blocks] = the end of the stream):
//   head    [head_beg, head_end)   from a to the end of a's block (or to b, when b lies in the same block); empty when a is a block start
//   blocks  [blk0, blk1)           the blocks that lie wholly inside [a, b): copied from the file
//   tail    [tail_beg, tail_end)   from the start of b's block to b; empty when b is a block start or the end of the stream
// a >= b: all three are empty.
struct Splice {
    uint64_t head_beg, head_end, tail_beg, tail_end;
    uint32_t blk0, blk1;
};

// the block that holds stream offset u < out_off[n_blocks]
SBX_SORT_HD uint32_t block_of(const uint64_t* out_off, uint32_t n_blocks, uint64_t u) {
    uint32_t lo = 0, hi = n_blocks;
    while (lo + 1 < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (out_off[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

SBX_SORT_HD Splice splice(uint64_t a, uint64_t b, const uint64_t* out_off, uint32_t n_blocks) {
    Splice s{a, a, b, b, 0u, 0u};
    const uint64_t total = out_off[n_blocks];
    if (b > total) b = total;
    if (a >= b) { s.tail_beg = s.tail_end = a; return s; }
    const uint32_t ba = block_of(out_off, n_blocks, a);
    const uint32_t bb = b >= total ? n_blocks : block_of(out_off, n_blocks, b);
    if (a == out_off[ba]) s.blk0 = ba;
    else {
        s.head_end = b < out_off[ba + 1] ? b : out_off[ba + 1];
        s.blk0 = ba + 1;
        if (s.head_end == b) { s.blk1 = s.blk0; s.tail_beg = s.tail_end = b; return s; }     // a and b in one block: one piece
    }
    s.blk1 = bb;
    s.tail_beg = out_off[bb];
    s.tail_end = b;
    return s;
}

}  // namespace slicec
}  // namespace sbx
