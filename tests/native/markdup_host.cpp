// markdup_host.cpp -- sambamba_amd/csrc/markdup_core.hpp on the CPU (tests/test_markdup_cpu.py): the 5' coordinate, the score, the keys
// and the header text of sbx_markdup, through the very functions the library compiles.
//   markdup_host ends              lines "pos reversed n_cigar (op len)* l_seq qual*" on stdin -> "coord score" per line
//   markdup_host poskeys REF_BITS  lines "library ref coord reversed" -> one key per line (decimal)
//   markdup_host pairkeys REF_BITS lines "library refA coordA revA scoreA refB coordB revB scoreB" (A: the earlier record) ->
//                                  "w0 w1 w2 end2" per line
//   markdup_host fits N_LIB N_REF  -> "1" / "0" and the reference bits
//   markdup_host header [CL]       header text on stdin -> the output header text (no CL: no @PG added); exit status 3 when refused
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/markdup_core.hpp"

int main(int argc, char** argv) {
    using namespace sbx::mdc;
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "ends") {
        long long pos, rev, n_cigar;
        while (scanf("%lld %lld %lld", &pos, &rev, &n_cigar) == 3) {
            std::vector<uint8_t> cigar(4 * (size_t)n_cigar + 1);
            for (long long k = 0; k < n_cigar; ++k) {
                long long op, len;
                if (scanf("%lld %lld", &op, &len) != 2) return 2;
                const uint32_t c = (uint32_t)len << 4 | (uint32_t)op;
                memcpy(cigar.data() + 1 + 4 * k, &c, 4);            // (an odd address, as in a record)
            }
            long long l_seq;
            if (scanf("%lld", &l_seq) != 1) return 2;
            std::vector<uint8_t> qual((size_t)l_seq + 1);
            for (long long k = 0; k < l_seq; ++k) { long long q; if (scanf("%lld", &q) != 1) return 2; qual[k] = (uint8_t)q; }
            printf("%d %u\n", five_prime_coord((int32_t)pos, rev != 0, cigar.data() + 1, (uint32_t)n_cigar), score_of(qual.data(), (uint32_t)l_seq));
        }
        return 0;
    }
    if (mode == "poskeys" && argc == 3) {
        const uint32_t ref_bits = (uint32_t)atoi(argv[2]);
        long long lib, ref, coord, rev;
        while (scanf("%lld %lld %lld %lld", &lib, &ref, &coord, &rev) == 4)
            printf("%llu\n", (unsigned long long)pos_key((int32_t)lib, (int32_t)ref, (int32_t)coord, (uint32_t)rev, ref_bits));
        return 0;
    }
    if (mode == "pairkeys" && argc == 3) {
        const uint32_t ref_bits = (uint32_t)atoi(argv[2]);
        long long lib, ra, ca, va, sa, rb, cb, vb, sb;
        while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &lib, &ra, &ca, &va, &sa, &rb, &cb, &vb, &sb) == 9) {
            uint64_t w[3], end2;
            pair_words(pos_key((int32_t)lib, (int32_t)ra, (int32_t)ca, (uint32_t)va, ref_bits), (uint32_t)sa,
                       pos_key((int32_t)lib, (int32_t)rb, (int32_t)cb, (uint32_t)vb, ref_bits), (uint32_t)sb, ref_bits, w, &end2);
            printf("%llu %llu %llu %llu\n", (unsigned long long)w[0], (unsigned long long)w[1], (unsigned long long)w[2], (unsigned long long)end2);
        }
        return 0;
    }
    if (mode == "fits" && argc == 4) {
        printf("%d %u\n", key_fits(atoi(argv[2]), atoi(argv[3])) ? 1 : 0, ref_bits_of(atoi(argv[3])));
        return 0;
    }
    if (mode == "header") {
        std::string in, out, why;
        char buf[4096];
        size_t k;
        while ((k = fread(buf, 1, sizeof buf, stdin)) > 0) in.append(buf, k);
        if (!markdup_header_text(in.data(), in.size(), argc > 2 ? argv[2] : nullptr, &out, &why)) { fprintf(stderr, "%s\n", why.c_str()); return 3; }
        fwrite(out.data(), 1, out.size(), stdout);
        return 0;
    }
    return 2;
}
