// sort_host.cpp -- sambamba_amd/csrc/sort_core.hpp on the CPU (tests/test_sort_core_cpu.py): the key K9a packs, the passes K9b runs and
// the header text sbx_sort_bam writes, through the very functions the library compiles.
//   sort_host keys N_REF        lines "ref pos flag" on stdin -> one key per line (decimal)
//   sort_host bits N_REF MAXPOS -> key_bits
//   sort_host passes VARYING    -> "n_passes key_bits shift..."
//   sort_host header            header text on stdin -> the output header text; exit status 3 when it is refused
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../sambamba_amd/csrc/sort_core.hpp"

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
