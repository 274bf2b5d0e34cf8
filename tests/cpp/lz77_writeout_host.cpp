// lz77_writeout_host -- the write-out of K1b (phase C of lz77_resolve_body, inflate.hip) on the CPU: lz::plan_writeout and lz::writeout_lane
// of csrc/lz77_copy.hpp are `__host__ __device__`; this program runs them batch by batch, 64 lanes one after the other, next to a model of
// the wave's window (base, the slide) and checks, for every alignment of the block's first byte:
//   * the stores of a block cover [0, isize) exactly, every byte once, with the right value, and touch nothing around the block;
//   * every 16-byte store goes to an address that is a multiple of 16, and single bytes are stored at most once in front of the first
//     aligned address and once behind the last one;
//   * what is carried from batch to batch is < 16 bytes, equals what the kernel derives from opos alone, and is still in the window:
//     the slide never drops a byte that is not in HBM yet.
//
//   g++ -O2 -std=c++17 -o lz77_writeout_host lz77_writeout_host.cpp && ./lz77_writeout_host      (prints "<blocks> <batches> 0")
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sambamba_amd/csrc/lz77_copy.hpp"

using namespace sbx;

namespace {

constexpr uint32_t kHist = 2048, kSpanMax = 1536, kCap = kHist + 1024u + kSpanMax;   // the geometry of k_lz77_resolve_exact
constexpr uint32_t kMargin = 64;

unsigned long long g_blocks = 0, g_batches = 0, g_bad = 0;

#define REQUIRE(c)                                                                                                  \
    do {                                                                                                            \
        if (!(c)) {                                                                                                 \
            if (g_bad++ < 20) fprintf(stderr, "line %d: %s  (a %u isize %u opos %u span %u)\n", __LINE__, #c, a, isize, opos, span); \
        }                                                                                                           \
    } while (0)

uint32_t rng_state = 0x5A4D0007u;
uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

// one block: its first byte at an address = a (mod 16), batches of the given spans
void run_block(uint32_t a, const std::vector<uint32_t>& spans) {
    uint32_t isize = 0;
    for (uint32_t s : spans) isize += s;
    std::vector<uint8_t> src(isize + 16);                         // the block's bytes (what phases A and B left in the window)
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(rnd() >> 11);
    // "HBM": 16-byte aligned storage, the block at offset kMargin + a, a sentinel around it
    std::vector<uint8_t> mem_raw(isize + 2 * kMargin + 64, 0xEE);
    uint8_t* mem = mem_raw.data() + ((16 - ((uintptr_t)mem_raw.data() & 15)) & 15);
    uint8_t* o = mem + kMargin + a;
    std::vector<uint8_t> count(isize + 2 * kMargin + 32, 0);      // stores per byte of mem
    std::vector<uint8_t> win(kCap + 16);                          // the wave's window: position `base` at win[0]
    uint32_t opos = 0, base = 0, wpos = 0, span = 0, heads = 0, tails = 0;
    ++g_blocks;
    for (size_t bi = 0; bi < spans.size(); ++bi) {
        span = spans[bi];
        const bool last = bi + 1 == spans.size();
        ++g_batches;
        // the slide of the kernel; it keeps [nb, opos)
        if (opos - base + kSpanMax > kCap) {
            const uint32_t nb = (opos - kHist) & ~15u;
            REQUIRE(opos - wpos < kHist - 16u);
            REQUIRE(nb <= wpos && nb >= base);
            base = nb;
        }
        REQUIRE(opos + span - base <= kCap);
        for (uint32_t p = base; p < opos + span; ++p) win[p - base] = src[p];
        for (uint32_t i = opos + span - base; i < win.size(); ++i) win[i] = 0xDD;      // (nothing behind the span is final)
        // the kernel does not carry wpos: it derives it from opos
        const uint32_t al = (a + opos) & ~15u, derived = al > a ? al - a : 0u;
        REQUIRE(derived == wpos);
        const lz::WritePlan wp = lz::plan_writeout(a, wpos, opos, span, last);
        const uint32_t end = opos + span;
        REQUIRE(wp.h_lo == wpos && wp.h_lo <= wp.g_lo && wp.g_lo <= wp.g_hi && wp.g_hi <= wp.t_hi && wp.t_hi <= end && wp.next == wp.t_hi);
        REQUIRE(wp.g_lo - wp.h_lo < 16u && wp.t_hi - wp.g_hi < 16u && (wp.g_hi - wp.g_lo) % 16u == 0);
        REQUIRE(wp.g_lo == wp.g_hi || (a + wp.g_lo) % 16u == 0);
        REQUIRE(wp.h_lo >= base);                                  // everything stored is in the window
        REQUIRE(last ? wp.next == end : end - wp.next < 16u);
        REQUIRE(wp.t_hi == wp.g_hi || last);
        heads += wp.g_lo != wp.h_lo;
        tails += wp.t_hi != wp.g_hi;
        for (uint32_t p = wp.g_lo; p < wp.g_hi; p += 16) REQUIRE(((uintptr_t)(o + p) & 15) == 0);
        for (uint32_t p = wp.h_lo; p < wp.t_hi; ++p) ++count[kMargin + a + p];
        for (uint32_t lane = 0; lane < 64; ++lane) lz::writeout_lane(wp, lane, win.data(), base, o);
        wpos = wp.next;
        opos = end;
    }
    REQUIRE(opos == isize && wpos == isize);
    REQUIRE(heads <= 1 && tails <= 1);
    for (uint32_t i = 0; i < count.size(); ++i) {
        const bool inside = i >= kMargin + a && i < kMargin + a + isize;
        REQUIRE(count[i] == (inside ? 1 : 0));
        REQUIRE(mem[i] == (inside ? src[i - kMargin - a] : 0xEE));
    }
}

}  // namespace

int main() {
    const uint32_t fixed[] = {1, 15, 16, 17, 1023, 1024, 1025, kSpanMax};
    const uint32_t totals[] = {0, 1, 15, 16, 17, 33, 65280, 65535};
    for (uint32_t a = 0; a < 16; ++a) {
        // batches of one size each, long enough for the window to slide several times; then each size as the only, the first and the last batch
        for (uint32_t s : fixed) {
            run_block(a, std::vector<uint32_t>(s < 64 ? 700 : 12, s));
            run_block(a, {s});
            for (uint32_t t : fixed) { run_block(a, {s, t}); run_block(a, {s, 1000, 7, t}); }
        }
        // random batch sizes (small ones as likely as large ones, empty batches too) adding up to a given block size
        for (uint32_t total : totals) {
            for (int rep = 0; rep < (total > 1000 ? 6 : 24); ++rep) {
                std::vector<uint32_t> spans;
                uint32_t left = total;
                while (left) {
                    const uint32_t r = rnd(), cap = (r & 3u) == 0 ? 20u : (r & 3u) == 1 ? 300u : kSpanMax;
                    uint32_t s = (r >> 8) % (cap + 1u);
                    if (s > left) s = left;
                    spans.push_back(s);
                    left -= s;
                }
                if (spans.empty() && rep % 2) spans.push_back(0);      // (an empty block has no batch, or one empty one)
                run_block(a, spans);
            }
        }
    }
    printf("%llu %llu %llu\n", g_blocks, g_batches, g_bad);
    return g_bad ? 1 : 0;
}
