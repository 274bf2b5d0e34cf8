// lz77_rounds_host -- the dependency rounds of K1b (phase B of lz77_resolve_body, inflate.hip) on the CPU, with the one-round fast path:
// the lock-step model of the rounds (batches of <= 64 entries and <= kSpan bytes, the window's slide, phase A, then rounds in which every
// read happens before the round's writes, the copies through the primitives of csrc/lz77_copy.hpp) run on token streams that
// tests/test_lz77_rounds_cpu.py writes with tests/deflate_build.py, against zlib's inflate of the same stream.  Per batch the predicate
// of the fast path is evaluated as the kernel does -- F = the start of the first pending match, lz::frontier_blocked per lane, no blocked
// lane = fast -- and then
//   * fast: ONE round with every pending lane ready and no ranges, searches or masks; the batch's bytes must equal zlib's right after it,
//     and the exact rule must agree that nothing was left to wait for (its masks, computed on the side, are all clear);
//   * otherwise: the exact rule as the kernel runs it (two branch-free binary searches per lane, rounds until no lane is pending).
// Prints a line per case: "<name> <one letter per batch: n = no near match, f = fast path, x = exact path> <rounds per batch, comma-separated>
// <entries per batch, comma-separated>";
// exit status 0 when every block equals zlib's bytes.
//
//   g++ -O2 -std=c++17 -o lz77_rounds_host lz77_rounds_host.cpp -lz && ./lz77_rounds_host CASES
//
// CASES: per case  u32 name length, name | u32 stream length, raw deflate stream | u32 n, n entries as K1a packs them
// (literal run << 24 | (dist - 1) << 9 | len) | u32 n, the block's literals.
#include <zlib.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../sambamba_amd/csrc/lz77_copy.hpp"

using namespace sbx;

namespace {

constexpr uint32_t kHist = 2048, kSpan = 1536, kCap = kHist + 1024u + kSpan;   // the geometry of k_lz77_resolve_exact

int g_bad = 0;
#define REQUIRE(c)                                                                                   \
    do {                                                                                             \
        if (!(c)) {                                                                                  \
            if (g_bad++ < 20) fprintf(stderr, "%s: line %d: %s\n", name.c_str(), __LINE__, #c);      \
            return false;                                                                            \
        }                                                                                            \
    } while (0)

// one ready match, copied as the kernel's round copies it; `writes` collects what the byte paths store (applied after every read of the round)
void copy_match(std::vector<uint8_t>& out, uint32_t dst, uint32_t dist, uint32_t len, std::vector<std::pair<uint32_t, uint8_t>>* writes) {
    const uint32_t src = dst - dist;
    if (dist < len && len <= 16 && dist <= 8) {
        const lz::W2 xx = lz::ld64(out.data() + src);
        lz::Short16 ws;
        lz::periodic16(xx.x, xx.y, len, lz::period_selector(dist, 0), lz::period_selector(dist, 1), lz::period_selector(dist, 2), lz::period_selector(dist, 3), &ws);
        ws.store(out.data() + dst, len);
        return;
    }
    for (uint32_t k = 0; k < len; ++k) writes->push_back({dst + k, out[src + k % dist]});      // reads [src, dst) only
}

bool run_case(const std::string& name, const std::vector<uint8_t>& stream, const std::vector<uint32_t>& ent, const std::vector<uint8_t>& lit_in,
              std::string* codes, std::string* rounds, std::string* takes) {
    std::vector<uint8_t> want(1u << 17);
    {
        z_stream z{};
        REQUIRE(inflateInit2(&z, -15) == Z_OK);
        z.next_in = (Bytef*)stream.data(); z.avail_in = (uInt)stream.size();
        z.next_out = want.data(); z.avail_out = (uInt)want.size();
        const int rc = inflate(&z, Z_FINISH);
        const size_t n = z.total_out;
        inflateEnd(&z);
        REQUIRE(rc == Z_STREAM_END && n <= 65536);
        want.resize(n);
    }
    const uint32_t isize = (uint32_t)want.size(), n_ent = (uint32_t)ent.size();
    std::vector<uint8_t> lit(lit_in);
    lit.resize(lit.size() + 64);                     // (the primitives may read a dword beyond a copy, as on the device)
    std::vector<uint8_t> out((size_t)isize + 64, 0);
    uint32_t opos = 0, lpos = 0, base = 0;
    for (uint32_t e0 = 0; e0 < n_ent;) {
        uint32_t take = 0, span = 0, lspan = 0;
        uint32_t lr[64], len[64], dist[64], dst[64], start[64], end[64];
        while (take < 64 && e0 + take < n_ent) {
            const uint32_t e = ent[e0 + take], l = e >> 24, n = e & 511u;
            if (span + l + n > kSpan) break;
            lr[take] = l; len[take] = n; dist[take] = ((e >> 9) & 0x7FFFu) + 1u;
            dst[take] = opos + span + l;
            span += l + n; lspan += l;
            ++take;
        }
        REQUIRE(take && opos + span <= isize);
        if (opos - base + kSpan > kCap) base = (opos - kHist) & ~15u;
        // phase A: literal runs, far matches
        uint64_t pending = 0;
        uint32_t lp = lpos;
        for (uint32_t j = 0; j < 64; ++j) {
            if (j >= take) { start[j] = end[j] = opos + span - base; continue; }
            REQUIRE(lp + lr[j] <= lit_in.size());
            for (uint32_t k = 0; k < lr[j]; ++k) out[dst[j] - lr[j] + k] = lit[lp++];
            if (len[j]) {
                REQUIRE(dist[j] <= dst[j]);
                const uint32_t src = dst[j] - dist[j];
                if (src < base) for (uint32_t k = 0; k < len[j]; ++k) out[dst[j] + k] = out[src + k];
                else pending |= 1ull << j;
            }
            start[j] = dst[j] - base; end[j] = dst[j] + len[j] - base;
        }
        // the exact rule's masks (the kernel computes them only where the fast path does not apply; here always, to compare)
        uint64_t dep[64];
        for (uint32_t i = 0; i < 64; ++i) {
            dep[i] = 0;
            if (!(pending >> i & 1)) continue;
            const uint32_t srco = dst[i] - dist[i] - base, s_hio = srco + (len[i] < dist[i] ? len[i] : dist[i]);
            uint32_t jlo = 0, jhi = 0;
            for (uint32_t step = 32; step; step >>= 1) {
                if (end[jlo + step - 1] <= srco) jlo += step;
                if (start[jhi + step - 1] < s_hio) jhi += step;
            }
            if (jhi > jlo) dep[i] = ((jhi >= 64 ? ~0ull : (1ull << jhi) - 1ull) & ~((1ull << jlo) - 1ull));
        }
        // the fast path's predicate, as the kernel evaluates it: one frontier, one test per lane, one ballot
        bool blocked = false;
        if (pending) {
            const uint32_t F = dst[__builtin_ctzll(pending)];
            for (uint32_t i = 0; i < take; ++i) {
                const uint32_t s_hi = dst[i] - dist[i] + (len[i] < dist[i] ? len[i] : dist[i]);
                blocked = blocked || lz::frontier_blocked(pending >> i & 1, s_hi, F);
            }
        }
        const bool fast = pending && !blocked;
        if (fast) for (uint32_t i = 0; i < 64; ++i) REQUIRE(!(dep[i] & pending));        // sufficient: the exact rule waits for nothing either
        uint32_t n_rounds = 0;
        codes->push_back(!pending ? 'n' : fast ? 'f' : 'x');
        while (pending) {
            REQUIRE(n_rounds < 64);
            uint64_t ready = 0;
            for (uint32_t i = 0; i < 64; ++i) if ((pending >> i & 1) && (fast || !(dep[i] & pending))) ready |= 1ull << i;
            REQUIRE(ready);
            lz::Short16 cp[64];
            for (uint32_t h = 0; h < 2; ++h) {            // plain matches of up to 32 bytes: all lanes load, then all lanes store, step by step
                for (uint32_t pass = 0; pass < 2; ++pass)
                    for (uint32_t i = 0; i < 64; ++i)
                        if ((ready >> i & 1) && dist[i] >= len[i] && len[i] <= 32) {
                            const uint32_t nn = len[i] > 16 * h ? (len[i] - 16 * h < 16 ? len[i] - 16 * h : 16) : 0;
                            if (pass == 0) cp[i].load(out.data() + dst[i] - dist[i] + 16 * h, nn);
                            else cp[i].store(out.data() + dst[i] + 16 * h, nn);
                        }
            }
            std::vector<std::pair<uint32_t, uint8_t>> writes;
            for (uint32_t i = 0; i < 64; ++i)
                if ((ready >> i & 1) && !(dist[i] >= len[i] && len[i] <= 32)) copy_match(out, dst[i], dist[i], len[i], &writes);
            for (auto& w : writes) out[w.first] = w.second;
            pending &= ~ready;
            ++n_rounds;
            if (fast) REQUIRE(!pending);                  // exactly one round
        }
        if (!rounds->empty()) { rounds->push_back(','); takes->push_back(','); }
        *rounds += std::to_string(n_rounds);
        *takes += std::to_string(take);
        // the batch's bytes are final now: zlib's
        for (uint32_t p = opos; p < opos + span; ++p) REQUIRE(out[p] == want[p]);
        opos += span; lpos += lspan; e0 += take;
    }
    REQUIRE(opos == isize);
    return true;
}

bool rd(FILE* f, void* p, size_t n) { return fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: lz77_rounds_host CASES\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    for (uint32_t n; rd(f, &n, 4);) {
        std::string name(n, ' ');
        std::vector<uint8_t> stream, lit;
        std::vector<uint32_t> ent;
        bool ok = rd(f, &name[0], n);
        ok = ok && rd(f, &n, 4); if (ok) stream.resize(n); ok = ok && rd(f, stream.data(), n);
        ok = ok && rd(f, &n, 4); if (ok) ent.resize(n); ok = ok && rd(f, ent.data(), 4ull * n);
        ok = ok && rd(f, &n, 4); if (ok) lit.resize(n); ok = ok && rd(f, lit.data(), n);
        if (!ok) { fprintf(stderr, "truncated case file\n"); return 2; }
        std::string codes, rounds, takes;
        if (!run_case(name, stream, ent, lit, &codes, &rounds, &takes)) ++g_bad;
        printf("%s %s %s %s\n", name.c_str(), codes.empty() ? "-" : codes.c_str(), rounds.empty() ? "-" : rounds.c_str(), takes.empty() ? "-" : takes.c_str());
    }
    fclose(f);
    return g_bad ? 1 : 0;
}
