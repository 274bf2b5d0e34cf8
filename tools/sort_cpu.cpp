// sort_cpu.cpp -- the CPU yardstick of `sbx-sort`: zlib inflates a BAM block by block on N threads, std::stable_sort
// orders the records by the key sbx-sort uses (sambamba_amd/csrc/sort_core.hpp), and zlib deflates the sorted stream in blocks of
// 0xFF00 bytes at the given level, again on N threads.  The header is copied as it is (the text is not re-serialised): a timing tool,
// not a test oracle (tests/sort_ref.py is that).  Prints the wall time of its phases on stderr.
//   make sort_cpu && ./sort_cpu [-t N] [-l LEVEL] [-n | -N] [-M] [--shuffle SEED] in.bam out.bam
// -n / -N / -M order by read name as `sbx-nsort` does: std::stable_sort under the comparators of namesort_core.hpp (-M: HI tag, then
// flag, among equal names); the yardstick of K14.
// --shuffle SEED writes the records in a seeded random order instead of the sorted one (makes the unsorted input of a measurement).
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../sambamba_amd/csrc/namesort_core.hpp"
#include "../sambamba_amd/csrc/sort_core.hpp"

namespace {
double now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
uint32_t rd32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }

template <class F>
void parallel_for(size_t n, int threads, F&& f) {
    std::vector<std::thread> pool;
    for (int t = 0; t < threads; ++t)
        pool.emplace_back([&, t] { for (size_t i = (size_t)t; i < n; i += (size_t)threads) f(i); });
    for (auto& th : pool) th.join();
}
}  // namespace

int main(int argc, char** argv) {
    int threads = 1, level = 1;
    bool shuffle = false, match_mates = false;
    uint32_t name_order = 0;
    uint64_t seed = 0;
    std::vector<std::string> files;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        if (a == "-t" && i + 1 < argc) threads = std::max(1, atoi(argv[++i]));
        else if (a == "-l" && i + 1 < argc) level = atoi(argv[++i]);
        else if (a == "-n") name_order = sbx::nsc::kOrderLex;
        else if (a == "-N") name_order = sbx::nsc::kOrderNatural;
        else if (a == "-M") match_mates = true;
        else if (a == "--shuffle" && i + 1 < argc) { shuffle = true; seed = strtoull(argv[++i], nullptr, 10); }
        else files.push_back(a);
    }
    if (files.size() != 2) { fprintf(stderr, "usage: sort_cpu [-t N] [-l LEVEL] [-n | -N] [-M] [--shuffle SEED] in.bam out.bam\n"); return 1; }
    const double t0 = now();
    // ---- read the file, find the blocks ----
    FILE* f = fopen(files[0].c_str(), "rb");
    if (!f) { perror(files[0].c_str()); return 1; }
    fseek(f, 0, SEEK_END);
    const size_t fsize = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> in(fsize);
    if (fread(in.data(), 1, fsize, f) != fsize) { fprintf(stderr, "short read\n"); return 1; }
    fclose(f);
    struct Blk { size_t off, clen; uint32_t isize; uint64_t uoff; };
    std::vector<Blk> blocks;
    uint64_t total = 0;
    for (size_t off = 0; off + 18 <= fsize;) {
        const size_t bsize = (size_t)(in[off + 16] | in[off + 17] << 8) + 1;        // BC subfield right behind XLEN = 6 (every BGZF writer)
        if (off + bsize > fsize) { fprintf(stderr, "truncated\n"); return 1; }
        const uint32_t isize = rd32(in.data() + off + bsize - 4);
        if (isize) { blocks.push_back({off + 18, bsize - 26, isize, total}); total += isize; }
        off += bsize;
    }
    const double t1 = now();
    // ---- inflate ----
    std::vector<uint8_t> u(total);
    bool bad = false;
    parallel_for(blocks.size(), threads, [&](size_t i) {
        z_stream z{};
        inflateInit2(&z, -15);
        z.next_in = in.data() + blocks[i].off; z.avail_in = (uInt)blocks[i].clen;
        z.next_out = u.data() + blocks[i].uoff; z.avail_out = blocks[i].isize;
        if (inflate(&z, Z_FINISH) != Z_STREAM_END) bad = true;
        inflateEnd(&z);
    });
    if (bad) { fprintf(stderr, "inflate failed\n"); return 1; }
    std::vector<uint8_t>().swap(in);
    const double t2 = now();
    // ---- records, keys, order ----
    if (total < 12 || memcmp(u.data(), "BAM\1", 4) != 0) { fprintf(stderr, "not a BAM\n"); return 1; }
    size_t p = 8 + rd32(u.data() + 4);
    const int32_t n_ref = (int32_t)rd32(u.data() + p);
    p += 4;
    for (int32_t r = 0; r < n_ref; ++r) p += 8 + rd32(u.data() + p);
    const size_t hlen = p;
    std::vector<uint64_t> off, key;
    while (p + 36 <= total) {
        const uint32_t bs = rd32(u.data() + p);
        off.push_back(p);
        key.push_back(sbx::sortc::sort_key((int32_t)rd32(u.data() + p + 4), (int32_t)rd32(u.data() + p + 8), rd32(u.data() + p + 16) >> 16, n_ref));
        p += 4 + (size_t)bs;
    }
    std::vector<uint32_t> perm(off.size());
    std::iota(perm.begin(), perm.end(), 0u);
    if (shuffle) { std::mt19937_64 rng(seed); std::shuffle(perm.begin(), perm.end(), rng); }
    else if (name_order) {
        namespace nsc = sbx::nsc;
        // the -M word of every record once (a record whose tags cannot be read counts as HI 0: a timing tool)
        std::vector<uint64_t> mate(off.size(), 0);
        if (match_mates)
            for (size_t i = 0; i < off.size(); ++i) {
                const uint8_t* rec = u.data() + off[i];
                nsc::NameFrame f;
                int32_t hi = 0;
                if (nsc::name_frame(rec, 4 + (uint64_t)rd32(rec), &f)) {
                    if (f.aux_ok) nsc::find_hi(rec, f.aux, 4 + (uint64_t)rd32(rec), &hi);
                    mate[i] = nsc::mate_word(hi, f.flag);
                }
            }
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
            const uint8_t *p = u.data() + off[a], *q = u.data() + off[b];
            const uint32_t np = p[12] ? p[12] - 1u : 0u, nq = q[12] ? q[12] - 1u : 0u;
            if (name_order == nsc::kOrderNatural) {
                const int c = nsc::mixed_str_compare(p + 36, np, q + 36, nq);
                return c != 0 ? c < 0 : mate[a] < mate[b];
            }
            if (nsc::name_less(p + 36, np, q + 36, nq)) return true;
            if (nsc::name_less(q + 36, nq, p + 36, np)) return false;
            return mate[a] < mate[b];
        });
    } else std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key[a] < key[b]; });
    const double t3 = now();
    // ---- the sorted stream ----
    std::vector<uint8_t> s(total);
    memcpy(s.data(), u.data(), hlen);
    size_t q = hlen;
    for (uint32_t i : perm) { const size_t n = 4 + (size_t)rd32(u.data() + off[i]); memcpy(s.data() + q, u.data() + off[i], n); q += n; }
    std::vector<uint8_t>().swap(u);
    const double t4 = now();
    // ---- deflate ----
    const size_t payload = 0xFF00, nb = (q + payload - 1) / payload;
    std::vector<std::vector<uint8_t>> out(nb);
    parallel_for(nb, threads, [&](size_t i) {
        const size_t b0 = i * payload, n = std::min(payload, q - b0);
        std::vector<uint8_t>& o = out[i];
        o.resize(65536);
        z_stream z{};
        deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
        z.next_in = s.data() + b0; z.avail_in = (uInt)n;
        z.next_out = o.data() + 18; z.avail_out = 65536 - 18 - 8;
        if (deflate(&z, Z_FINISH) != Z_STREAM_END) bad = true;
        const size_t clen = z.total_out;
        deflateEnd(&z);
        const uint8_t hd[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        memcpy(o.data(), hd, 16);
        const uint16_t bsz = (uint16_t)(clen + 25);
        memcpy(o.data() + 16, &bsz, 2);
        const uint32_t crc = (uint32_t)crc32(crc32(0, nullptr, 0), s.data() + b0, (uInt)n), isz = (uint32_t)n;
        memcpy(o.data() + 18 + clen, &crc, 4);
        memcpy(o.data() + 22 + clen, &isz, 4);
        o.resize(clen + 26);
    });
    if (bad) { fprintf(stderr, "deflate failed (incompressible block)\n"); return 1; }
    const double t5 = now();
    FILE* g = fopen(files[1].c_str(), "wb");
    if (!g) { perror(files[1].c_str()); return 1; }
    for (auto& o : out) fwrite(o.data(), 1, o.size(), g);
    const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    fwrite(eof, 1, 28, g);
    if (fclose(g) != 0) { fprintf(stderr, "error writing\n"); return 1; }
    const double t6 = now();
    fprintf(stderr, "sort_cpu: %zu records, %llu inflated bytes, %d thread(s), level %d%s: read %.1f ms, inflate %.1f ms, keys + %s %.1f ms, "
                    "gather %.1f ms, deflate %.1f ms, write %.1f ms, total %.1f ms\n", perm.size(), (unsigned long long)total, threads, level,
            shuffle ? " (shuffle)" : "", (t1 - t0) * 1e3, (t2 - t1) * 1e3, shuffle ? "shuffle" : "stable_sort", (t3 - t2) * 1e3, (t4 - t3) * 1e3,
            (t5 - t4) * 1e3, (t6 - t5) * 1e3, (t6 - t0) * 1e3);
    return 0;
}
