// subsample.hip -- K22: the coverage of every reference position over a WHOLE file, and from it the verdict of `subsample --type
// fasthash --max-cov N` per record (engine_subsample.cpp; the arithmetic is subsample_core.hpp, the definition DESIGN.md section 8).
// The file passes through the device twice (K1 + K2 in batches both times); the coverage array D stays resident in between: one
// uint32 per position of every reference plus one per reference, ~12.4 GB for a human genome.
//
//   K22a k_cov_mark     first pass, one lane per described record of a batch: flag, ref_id, pos and CIGAR read from U where K1 left
//                       them, checked against block_size and the batch end as K16b checks them; a counted record adds +1 at the slot
//                       of its pos and 0xFFFFFFFF (-1) at the slot of its e with two ordinary atomicAdd.  Both slots lie inside the
//                       record's own reference (subc::record_span), so the bound of every atomic is the array's.  Counted and
//                       malformed records are counted once per wave.
//   K22b k_cov_tile_sum, launch_scan64, k_cov_tile_scan
//                       between the passes: D scanned in place, inclusive, modulo 2^32.  Tiles of subc::kCovTile words; the first
//                       kernel adds every tile up in 64 bits, launch_scan64 (one workgroup, scan.hip) turns the sums into tile bases,
//                       the second kernel scans every tile again from its base and stores.  16 bytes per lane both ways, consecutive
//                       lanes on consecutive 16 bytes.  D is allocated in whole tiles and zeroed, so no load or store needs a bound.
//   K22c k_cov_verdict  second pass, one lane per record: the span once more, D at the slot of pos and of e - 1, the FNV-1a hash of
//                       the name (viewc::name_seed_hash, seed 0), subc::keeps.  With -r the verdict goes to count[] for K21
//                       (PackArgs::count), without it the new flag word of a dropped record goes to patch[] (PackArgs::bin at byte
//                       18).  Bytes to write, records over the cap, records dropped and the largest coverage are accumulated once
//                       per wave (the bytes once per workgroup).
//
// Bytes moved.  K22a: 32 (descriptor) + 36 + name length + CIGAR per record, scattered by record, and two 4-byte atomics per counted
// record; deep pile-ups put many atomics of a batch on few addresses -- the suspected cost on 300x data, NOT measured.  K22b: 4 bytes
// read per slot by the sums, 4 read + 4 written by the rescan = 12 bytes per slot, plus 16 bytes per tile of sums; at the 6.3 TB/s a
// float4 copy reaches on this part (8 TB/s peak HBM3E) the 3.1e9 slots of a human genome are 37.2 GB and ~6 ms; NOT measured.  The
// hipMemset in front of the first pass writes 4 more bytes per slot.  K22c: what K22a reads, plus the name, plus two 4-byte loads of
// D per counted record (neighbours in a sorted file share cache lines), and 4 bytes written per record.  No LDS atomics; LDS holds
// one row of wave sums per workgroup.  NOTHING here has a measured time.
#include "subsample.hpp"

#include "common.hpp"
#include "scan.hpp"
#include "view_core.hpp"
#include "wave_prims.hpp"

namespace sbx {

namespace {

// the span of record i of the batch; false: the record is malformed (nothing of it may be used)
__device__ __forceinline__ bool span_of(const CovArgs& a, uint64_t i, const uint8_t** rec, subc::Span* s) {
    const uint64_t rec_off = a.desc[i].rec_off;
    if (rec_off + 36 > a.u_end) return false;
    const uint8_t* p = a.U + rec_off;
    const uint32_t bs = ld32(p);
    if (!record_len_ok(bs, rec_off, a.u_end)) return false;
    *rec = p;
    return subc::record_span(p, bs, a.base, a.n_ref, s);
}

__global__ __launch_bounds__(kCovThreads) void k_cov_mark(CovArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * kCovThreads + threadIdx.x;
    bool bad = false, counted = false;
    if (i < a.n) {
        const uint8_t* rec;
        subc::Span s;
        bad = !span_of(a, i, &rec, &s);
        if (!bad && s.counted) {
            counted = true;
            atomicAdd(a.D + s.lo, 1u);
            atomicAdd(a.D + s.hi, 0xFFFFFFFFu);
        }
    }
    const unsigned long long mb = __ballot(bad), mc = __ballot(counted);
    if ((threadIdx.x & 63u) == 0) {
        if (mb) atomicAdd(a.acc + kCovBad, (unsigned long long)__popcll(mb));
        if (mc) atomicAdd(a.acc + kCovCounted, (unsigned long long)__popcll(mc));
    }
}

// ---- K22b: a tile is kCovRounds rounds of kCovThreads lanes x 4 words ----
constexpr uint32_t kCovRounds = subc::kCovTile / (kCovThreads * 4);
static_assert(kCovRounds * kCovThreads * 4 == subc::kCovTile, "a tile is whole rounds of 16 bytes per lane");

__global__ __launch_bounds__(kCovThreads) void k_cov_tile_sum(const uint32_t* __restrict__ D, uint64_t* __restrict__ tile_sum) {
    __shared__ unsigned long long w_sum[kCovThreads / 64];
    const uint64_t tile = blockIdx.x;
    const uint4* q = (const uint4*)(D + tile * subc::kCovTile);
    unsigned long long s = 0;
#pragma unroll
    for (uint32_t k = 0; k < kCovRounds; ++k) {
        const uint4 v = q[k * kCovThreads + threadIdx.x];
        s += (unsigned long long)v.x + v.y + v.z + v.w;
    }
    s = block_sum<unsigned long long>(s, w_sum);
    if (threadIdx.x == 0) tile_sum[tile] = s;
}

// tile_base: the exclusive scan of the tile sums; only its low 32 bits matter to a word of D
__global__ __launch_bounds__(kCovThreads) void k_cov_tile_scan(uint32_t* __restrict__ D, const uint64_t* __restrict__ tile_base) {
    __shared__ uint32_t w_sum[kCovThreads / 64];
    const uint64_t tile = blockIdx.x;
    uint4* q = (uint4*)(D + tile * subc::kCovTile);
    uint32_t carry = (uint32_t)tile_base[tile];
#pragma unroll
    for (uint32_t k = 0; k < kCovRounds; ++k) {
        uint4 v = q[k * kCovThreads + threadIdx.x];
        uint32_t total;
        const uint32_t before = carry + block_exclusive<uint32_t>(v.x + v.y + v.z + v.w, w_sum, &total);
        v.x += before; v.y += v.x; v.z += v.y; v.w += v.z;
        q[k * kCovThreads + threadIdx.x] = v;
        carry += total;
    }
}

__global__ __launch_bounds__(kCovThreads) void k_cov_verdict(CovArgs a) {
    __shared__ unsigned long long w_sum[kCovThreads / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kCovThreads + threadIdx.x;
    bool bad = false, over = false, dropped = false;
    unsigned long long len = 0, cov_seen = 0;
    if (i < a.n) {
        const uint8_t* rec;
        subc::Span s;
        bad = !span_of(a, i, &rec, &s);
        uint32_t patch = streamc::kNoPatch;
        if (!bad) {
            if (s.counted) {
                const uint32_t c0 = a.D[s.lo], c1 = a.D[s.hi - 1];
                const uint32_t cov = c0 > c1 ? c0 : c1;
                cov_seen = cov;
                over = cov > a.max_cov;
                if (over) {         // (cov <= max_cov keeps whatever the hash)
                    const uint32_t h = (uint32_t)viewc::name_seed_hash(rec + 36, s.name_len, 0);
                    dropped = !subc::keeps(h, cov, a.max_cov);
                }
            }
            if (dropped) patch = (s.flag | subc::kDroppedFlag) & 0xFFFFu;
            if (!(a.count && dropped)) len = s.bs + 4ull;
        }
        if (a.count) a.count[i] = bad || dropped ? 0u : 1u;
        if (a.patch) a.patch[i] = patch;
    }
    const unsigned long long bytes = block_sum<unsigned long long>(len, w_sum);
    const unsigned long long mb = __ballot(bad), mo = __ballot(over), md = __ballot(dropped);
    cov_seen = wave_max(cov_seen);
    if ((threadIdx.x & 63u) == 0) {
        if (mb) atomicAdd(a.acc + kCovBad, (unsigned long long)__popcll(mb));
        if (mo) atomicAdd(a.acc + kCovOver, (unsigned long long)__popcll(mo));
        if (md) atomicAdd(a.acc + kCovDropped, (unsigned long long)__popcll(md));
        if (cov_seen) atomicMax(a.acc + kCovMaxSeen, cov_seen);
    }
    if (threadIdx.x == 0 && bytes) atomicAdd(a.acc + kCovBytes, bytes);
}

}  // namespace

void launch_cov_mark(const CovArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_cov_mark, dim3(cov_groups(a.n)), dim3(kCovThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

void launch_cov_scan(uint32_t* D, uint64_t n_tiles, uint64_t* tile_sum, hipStream_t stream) {
    if (!n_tiles) return;
    // one workgroup per tile: a grid of kMaxCovTiles x kCovThreads threads stays below 2^32 (68e9 slots, 275 GB of D)
    if (n_tiles > kMaxCovTiles) throw Error(SBX_EUNSUPPORTED, "the references hold more positions than the coverage scan takes");
    hipLaunchKernelGGL(k_cov_tile_sum, dim3((uint32_t)n_tiles), dim3(kCovThreads), 0, stream, D, tile_sum);
    SBX_HIP(hipGetLastError());
    launch_scan64(tile_sum, n_tiles, 0, stream);
    hipLaunchKernelGGL(k_cov_tile_scan, dim3((uint32_t)n_tiles), dim3(kCovThreads), 0, stream, D, tile_sum);
    SBX_HIP(hipGetLastError());
}

void launch_cov_verdict(const CovArgs& a, hipStream_t stream) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_cov_verdict, dim3(cov_groups(a.n)), dim3(kCovThreads), 0, stream, a);
    SBX_HIP(hipGetLastError());
}

}  // namespace sbx
