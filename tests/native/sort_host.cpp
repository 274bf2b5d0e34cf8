// sort_host.cpp -- sambamba_amd/csrc/sort_core.hpp on the CPU (tests/test_sort_core_cpu.py): the key K9a packs, the passes K9b runs and
// the header text sbx_sort_bam writes, through the very functions the library compiles.
//   sort_host keys N_REF        lines "ref pos flag" on stdin -> one key per line (decimal)
//   sort_host bits N_REF MAXPOS -> key_bits
//   sort_host passes VARYING    -> "n_passes key_bits shift..."
//   sort_host header            header text on stdin -> the output header text; exit status 3 when it is refused
//   sort_host pieces HLEN CAP   record lengths on stdin -> the stream of HLEN header bytes + the records, assembled piece by piece (CAP
//                               bytes each) the way the output tail does it: first_record_ending_behind for the bounds, piece_records
//                               for the records of a piece, clip_to_piece for the bytes of each.  stdout: the pieces one behind the
//                               other.  stderr: "bounds b0 b1 ..." and per piece "piece k p0 p1 r0 r1 unwritten twice outside" --
//                               bytes of [0, p1 - p0) written never / more than once, writes outside it.  Header byte j is
//                               header_byte(j), byte j of record i record_byte(i, j).
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/sort_core.hpp"

static uint8_t header_byte(uint64_t j) { return (uint8_t)(0x80 | (j % 127)); }
static uint8_t record_byte(uint64_t i, uint64_t j) { return (uint8_t)((i * 131 + j * 7 + 3) % 127); }

static int pieces(uint64_t hlen, uint64_t cap) {
    using namespace sbx::sortc;
    if (!cap) return 2;
    std::vector<uint64_t> off, out_off;            // the record's place in the store, and in the stream
    std::vector<uint8_t> store;
    unsigned long long l;
    out_off.push_back(hlen);
    while (scanf("%llu", &l) == 1) {
        const uint64_t i = off.size();
        off.push_back(store.size());
        for (uint64_t j = 0; j < l; ++j) store.push_back(record_byte(i, j));
        out_off.push_back(out_off.back() + l);
    }
    const uint64_t n = off.size(), total = out_off.back();
    out_off.push_back(0);                          // (n + 2 words, as on the device)
    const size_t n_bounds = (size_t)((total + cap - 1) / cap) + 1;
    std::vector<uint32_t> bounds(n_bounds, (uint32_t)n);
    if (n) for (size_t k = 0; k < n_bounds; ++k) bounds[k] = (uint32_t)first_record_ending_behind(out_off.data(), n, (uint64_t)k * cap);
    fprintf(stderr, "bounds");
    for (uint32_t b : bounds) fprintf(stderr, " %u", b);
    fprintf(stderr, "\n");
    const uint64_t guard = 64;                     // room on both sides of the piece: a write there is counted, not made elsewhere
    std::vector<uint8_t> buf(cap + 2 * guard);
    std::vector<uint32_t> cnt(cap + 2 * guard);
    for (uint64_t p0 = 0, k = 0; p0 < total; p0 += cap, ++k) {
        const uint64_t p1 = std::min(total, p0 + cap);
        std::fill(buf.begin(), buf.end(), (uint8_t)0xEE);
        std::fill(cnt.begin(), cnt.end(), 0u);
        uint64_t outside = 0;
        auto put = [&](uint64_t at, uint8_t v) {   // byte `at` of the piece; `at` is unsigned: below zero shows as huge
            if (at >= p1 - p0) ++outside;
            const uint64_t g = at + guard;
            if (g < buf.size()) { buf[g] = v; ++cnt[g]; }
        };
        if (p0 < hlen) {
            const uint64_t he = std::min(hlen, p1);
            for (uint64_t j = p0; j < he; ++j) put(j - p0, header_byte(j));
        }
        uint64_t r0, r1;
        piece_records(bounds.data(), (size_t)k, n, &r0, &r1);
        for (uint64_t i = r0; i < r1; ++i) {
            PieceClip c;
            if (!clip_to_piece(out_off[i], out_off[i + 1], p0, p1, &c)) continue;
            for (uint64_t b = 0; b < c.len; ++b) put(c.dst + b, store[off[i] + c.src + b]);
        }
        uint64_t unwritten = 0, twice = 0;
        for (uint64_t j = 0; j < p1 - p0; ++j) { unwritten += cnt[guard + j] == 0; twice += cnt[guard + j] > 1; }
        fprintf(stderr, "piece %llu %llu %llu %llu %llu %llu %llu %llu\n", (unsigned long long)k, (unsigned long long)p0, (unsigned long long)p1,
                (unsigned long long)r0, (unsigned long long)r1, (unsigned long long)unwritten, (unsigned long long)twice, (unsigned long long)outside);
        fwrite(buf.data() + guard, 1, (size_t)(p1 - p0), stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    using namespace sbx::sortc;
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "keys" && argc == 3) {
        const int n_ref = atoi(argv[2]);
        long long ref, pos, flag;
        while (scanf("%lld %lld %lld", &ref, &pos, &flag) == 3)
            printf("%llu\n", (unsigned long long)sort_key((int32_t)ref, (int32_t)pos, (uint32_t)flag, n_ref));
        return 0;
    }
    if (mode == "bits" && argc == 4) {
        printf("%u\n", key_bits(atoi(argv[2]), atoll(argv[3])));
        return 0;
    }
    if (mode == "passes" && argc == 3) {
        uint32_t shift[8], bits = 0;
        const uint32_t n = plan_passes(strtoull(argv[2], nullptr, 0), shift, &bits);
        printf("%u %u", n, bits);
        for (uint32_t k = 0; k < n; ++k) printf(" %u", shift[k]);
        printf("\n");
        return 0;
    }
    if (mode == "pieces" && argc == 4) return pieces(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    if (mode == "header") {
        std::string in, out, why;
        char buf[4096];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, stdin)) > 0) in.append(buf, k);
        if (!sort_header_text(in.data(), in.size(), &out, &why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
        fwrite(out.data(), 1, out.size(), stdout);
        return 0;
    }
    return 2;
}
