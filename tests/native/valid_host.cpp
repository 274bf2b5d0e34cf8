// valid_host.cpp -- validc::record_mask (sambamba_amd/csrc/valid_core.hpp) on the CPU, for tests/test_valid_core_cpu.py.
//
//   valid_host masks   stdin: one record per line as hex ("-": no bytes).  Every record is copied into a heap block of exactly its
//                      length (so AddressSanitizer sees a read one byte past it) and, for the plain build, once more in front of
//                      64 guard bytes that are checked afterwards.  stdout: one mask per line.
//   valid_host cuts    the same input; per record one line with the masks of its first n bytes for n = 0 .. length, the avail
//                      argument cut with them.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/valid_core.hpp"

namespace {

std::vector<uint8_t> from_hex(const std::string& s) {
    std::vector<uint8_t> out;
    if (s == "-") return out;
    auto nib = [](char c) { return c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10; };
    for (size_t k = 0; k + 1 < s.size(); k += 2) out.push_back((uint8_t)(nib(s[k]) << 4 | nib(s[k + 1])));
    return out;
}

// the mask of the first n bytes of r, read from a block of exactly n bytes
unsigned mask_of(const std::vector<uint8_t>& r, size_t n) {
    uint8_t* exact = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(exact, r.data(), n);
    const unsigned m = sbx::validc::record_mask(exact, n);
    free(exact);
    // behind guard bytes that a stray read would take for a NUL, a tag or a quality
    for (int fill : {0x00, 0xFF, 0x5A}) {
        std::vector<uint8_t> g(n + 64, (uint8_t)fill);
        if (n) memcpy(g.data(), r.data(), n);
        if (sbx::validc::record_mask(g.data(), n) != m) {
            fprintf(stderr, "the mask of %zu bytes depends on the bytes behind them (guard %02x)\n", n, fill);
            exit(2);
        }
    }
    return m;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 1;
    const std::string mode = argv[1];
    std::string line;
    while (std::getline(std::cin, line)) {
        const std::vector<uint8_t> r = from_hex(line);
        if (mode == "masks") printf("%u\n", mask_of(r, r.size()));
        else {
            for (size_t n = 0; n <= r.size(); ++n) printf(n ? " %u" : "%u", mask_of(r, n));
            printf("\n");
        }
    }
    return 0;
}
