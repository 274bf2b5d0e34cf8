// view_host.cpp -- sambamba_amd/csrc/view_core.hpp on the CPU (tests/test_view_core_cpu.py): the overlap predicate, the subsampling
// hash and threshold and the flag test K12 evaluates, the --num-filter parser and the text of -I, through the very functions the
// library compiles.
//   view_host overlap           lines "ref pos covered r_ref r_start r_end" on stdin (r_ref 4294967295: "*") -> 0 / 1 per line
//   view_host flags             lines "flag set unset" on stdin -> 0 / 1 per line
//   view_host hash SEED         lines of hex-encoded names on stdin ("-": the empty name) -> one hash per line (decimal)
//   view_host threshold FRAC    -> the threshold; exit status 3 when the fraction is refused
//   view_host numfilter TEXT    -> "set unset"; exit status 3 when the text is refused
//   view_host json [HEXNAME LENGTH]...   -> the text of -I
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/view_core.hpp"

static std::string unhex(const std::string& h) {
    std::string out;
    if (h == "-") return out;
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)strtoul(h.substr(k, 2).c_str(), nullptr, 16));
    return out;
}

int main(int argc, char** argv) {
    using namespace sbx::viewc;
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "overlap" && argc == 2) {
        long long ref, pos, cov, rr, rs, re;
        while (scanf("%lld %lld %lld %lld %lld %lld", &ref, &pos, &cov, &rr, &rs, &re) == 6)
            printf("%d\n", overlaps((int32_t)ref, (int32_t)pos, (uint32_t)cov, (uint32_t)rr, (uint32_t)rs, (uint32_t)re) ? 1 : 0);
        return 0;
    }
    if (mode == "flags" && argc == 2) {
        unsigned flag, set, unset;
        while (scanf("%u %u %u", &flag, &set, &unset) == 3) printf("%d\n", flags_pass(flag, set, unset) ? 1 : 0);
        return 0;
    }
    if (mode == "hash" && argc == 3) {
        const uint64_t seed = strtoull(argv[2], nullptr, 10);
        char line[1024];
        while (scanf("%1023s", line) == 1) {
            const std::string name = unhex(line);
            const uint64_t h = name_seed_hash((const uint8_t*)name.data(), (uint32_t)name.size(), seed);
            printf("%llu\n", (unsigned long long)h);
        }
        return 0;
    }
    if (mode == "threshold" && argc == 3) {
        uint64_t t = 0;
        if (!subsample_threshold(strtod(argv[2], nullptr), &t)) return 3;
        printf("%llu\n", (unsigned long long)t);
        return 0;
    }
    if (mode == "numfilter" && argc == 3) {
        uint16_t a = 0, b = 0;
        if (!parse_num_filter(argv[2], &a, &b)) return 3;
        printf("%u %u\n", (unsigned)a, (unsigned)b);
        return 0;
    }
    if (mode == "json" && argc % 2 == 0) {
        std::vector<std::string> names;
        std::vector<int64_t> lengths;
        for (int k = 2; k + 1 < argc; k += 2) { names.push_back(unhex(argv[k])); lengths.push_back(atoll(argv[k + 1])); }
        const std::string t = reference_info_json(names, lengths);
        fwrite(t.data(), 1, t.size(), stdout);
        return 0;
    }
    return 2;
}
