// subsample_host.cpp -- subsample_core.hpp compiled for the host (tests/test_subsample_core_cpu.py), plainly and under ASan + UBSan.
//   subsample_host keeps    stdin: "h cov max_cov" per line (decimal); prints 1 or 0 per line: subc::keeps
//   subsample_host slots    stdin: "n_ref LN..." per line; prints base[0 .. n_ref] and the tiles of the scan
//   subsample_host span     stdin: "n_ref LN... HEX" per line, HEX the bytes of one record from its block_size field on, in a buffer
//                           of exactly that size (the sanitizers see a read behind it); prints "bad", "uncounted NAME_LEN" or
//                           "counted LO HI NAME_LEN FLAG" (slots of pos and of e in the coverage array): subc::record_span
//   subsample_host parts    stdin: "flag ref_id n_ref pos ln bases" per line; prints counted (0 / 1) and, when counted, e:
//                           subc::counted and subc::span_end on their own, for values no record of a test file can carry
//   subsample_host tile     prints subc::kCovTile
// Exit 0; 2: usage or unreadable input.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/subsample_core.hpp"

using namespace sbx;

namespace {

bool read_refs(std::istringstream& in, std::vector<int32_t>* ln) {
    long n = 0;
    if (!(in >> n) || n < 0) return false;
    ln->resize((size_t)n);
    for (long r = 0; r < n; ++r) {
        long long v;
        if (!(in >> v)) return false;
        (*ln)[(size_t)r] = (int32_t)v;
    }
    return true;
}

int hex_of(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; }

}  // namespace

int main(int argc, char** argv) {
    const std::string mode = argc >= 2 ? argv[1] : "";
    if (mode == "tile") { printf("%u\n", subc::kCovTile); return 0; }
    if (mode != "keeps" && mode != "slots" && mode != "span" && mode != "parts") {
        fprintf(stderr, "usage: subsample_host keeps|slots|span|parts|tile\n");
        return 2;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        if (mode == "keeps") {
            unsigned long long h, cov, max_cov;
            if (!(in >> h >> cov >> max_cov)) return 2;
            printf("%d\n", subc::keeps((uint32_t)h, (uint32_t)cov, (uint32_t)max_cov) ? 1 : 0);
        } else if (mode == "parts") {
            unsigned long long flag, bases;
            long long ref_id, n_ref, pos, ln;
            if (!(in >> flag >> ref_id >> n_ref >> pos >> ln >> bases)) return 2;
            const bool c = subc::counted((uint32_t)flag, (int32_t)ref_id, (int32_t)n_ref, (int32_t)pos, ln);
            if (c) printf("1 %u\n", subc::span_end((int32_t)pos, (uint32_t)bases, ln));
            else printf("0\n");
        } else {
            std::vector<int32_t> ln;
            if (!read_refs(in, &ln)) return 2;
            const std::vector<uint64_t> base = subc::slot_bases(ln.data(), ln.size());
            if (mode == "slots") {
                for (uint64_t b : base) printf("%llu ", (unsigned long long)b);
                printf("%llu\n", (unsigned long long)subc::cov_tiles(base.back()));
                continue;
            }
            std::string hex;
            if (!(in >> hex) || hex.size() % 2 || hex.size() < 2 * 36) return 2;
            std::vector<uint8_t> rec(hex.size() / 2);          // exactly the record: a read behind it is the sanitizer's to report
            for (size_t k = 0; k < rec.size(); ++k) {
                const int a = hex_of(hex[2 * k]), b = hex_of(hex[2 * k + 1]);
                if (a < 0 || b < 0) return 2;
                rec[k] = (uint8_t)(a << 4 | b);
            }
            const uint32_t bs = subc::load32(rec.data());
            if (bs < 32 || 4ull + bs != rec.size()) return 2;   // (the caller's check: record_len_ok)
            subc::Span s;
            if (!subc::record_span(rec.data(), bs, base.data(), (int32_t)ln.size(), &s)) printf("bad\n");
            else if (!s.counted) printf("uncounted %u\n", s.name_len);
            else printf("counted %llu %llu %u %u\n", (unsigned long long)s.lo, (unsigned long long)s.hi, s.name_len, s.flag);
        }
    }
    return 0;
}
