// scan.hpp -- the device scans every command shares (scan.hip): counts to offsets, lengths to offsets, and the two one-line fills.
// Which shapes the tests reach: DESIGN.md, "The scan layer".
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace sbx {

// d_base[i] = sum of d_count[j], j < i, for i in [0, n]: one workgroup, rounds of 4096 counts, the sum carried between rounds
void launch_count_scan(const uint32_t* d_count, uint32_t n, uint64_t* d_base, hipStream_t stream);
// in place, one workgroup, rounds of 1024 values: x[i] = first + sum of x[j], j < i, for i in [0, m] -- m + 1 words are written,
// m == 0 writes x[0] = first
void launch_scan64(uint64_t* d_x, uint64_t m, uint64_t first, hipStream_t stream);

// d_out_off[i] = first + sum of d_len[d_perm[j]], j < i, for i in [0, n]; d_perm == nullptr: the identity.  n == 0 writes nothing.
constexpr uint32_t kLenTile = 2048;
inline size_t len_tiles(uint64_t n) { return (size_t)((n + kLenTile - 1) / kLenTile); }
void launch_sorted_offsets(const uint32_t* d_len, const uint32_t* d_perm, uint64_t n, uint64_t first, uint64_t* d_tile_sum /* len_tiles + 2 */,
                           uint64_t* d_out_off, hipStream_t stream);

// The other way to the same offsets, for a kernel that measures one item per lane and sums its workgroup itself (K13a, K15b): it runs
// with kGroupThreads threads and stores the sum of workgroup g in group_sum[g]; launch_scan64(group_sum, groups(n), 0) makes the bases;
// then d_off[i] = first + d_group_base[i / kGroupThreads] + the lengths in front of i inside its group, i < n, and d_off[n] = first + all.
constexpr uint32_t kGroupThreads = 256;
inline uint32_t group_count(uint64_t n) { return (uint32_t)((n + kGroupThreads - 1) / kGroupThreads); }
void launch_group_offsets(const uint32_t* d_len, const uint64_t* d_group_base, uint64_t n, uint64_t first, uint64_t* d_off, hipStream_t stream);

// d_val[i] = i, and d[i] = v, for i < n
void launch_iota(uint32_t* d_val, uint64_t n, hipStream_t stream);
void launch_fill32(uint32_t* d, uint32_t v, uint64_t n, hipStream_t stream);

}  // namespace sbx
