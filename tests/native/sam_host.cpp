// sam_host.cpp -- sambamba_amd/csrc/sam_core.hpp on the CPU (tests/test_sam_core_cpu.py): the statements K13 runs, through the very
// functions the library compiles.
//   sam_host g SEED N      %g of floats against snprintf("%g", (double)f) of this machine's C library: every exponent with the edge
//                          mantissas and 64 random ones, both signs; k * 10^p (k = 1 .. 9999, p = -10 .. 10) and its neighbours; the
//                          floats around 999999.5 * 10^p; N random bit patterns.  Prints the first mismatches and "checked C bad B".
//   sam_host lines         stdin: a line with the hex-encoded reference names ("-": none), then one hex-encoded record per line.
//                          Per record: "status length emit_status guards hexline" -- sam_line_length, then sam_line_emit into a
//                          buffer of exactly that length between two guards of 64 bytes (guards: 1 = untouched).  The record lies
//                          in an allocation of exactly its size, so a sanitizer build sees every read behind it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/sam_core.hpp"

using namespace sbx::samc;

static uint64_t rng_state;
static uint64_t rng() {                              // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static unsigned long long n_checked = 0, n_bad = 0;
static void check_bits(uint32_t bits) {
    float f;
    memcpy(&f, &bits, 4);
    char want[64];
    snprintf(want, sizeof want, "%g", (double)f);
    const Text16 t = g_format(bits);
    char got[17] = {0};
    for (uint32_t k = 0; k < t.n && k < 16; ++k) got[k] = (char)((k < 8 ? t.lo >> (8 * k) : t.hi >> (8 * (k - 8))) & 0xFF);
    ++n_checked;
    if (strcmp(want, got) != 0 && n_bad++ < 20) printf("mismatch bits=%08x want=%s got=%s\n", bits, want, got);
}
static void check_around(float f) {
    uint32_t b;
    memcpy(&b, &f, 4);
    for (int d = -2; d <= 2; ++d) { check_bits(b + (uint32_t)d); check_bits((b + (uint32_t)d) | 0x80000000u); }
}

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    out.reserve(h.size() / 2);
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((uint8_t)(v(h[k]) << 4 | v(h[k + 1])));
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "g" && argc == 4) {
        rng_state = strtoull(argv[2], nullptr, 10);
        const unsigned long long n_random = strtoull(argv[3], nullptr, 10);
        for (uint32_t e = 0; e < 256; ++e)
            for (uint32_t sign = 0; sign < 2; ++sign) {
                const uint32_t head = sign << 31 | e << 23;
                for (uint32_t m : {0u, 1u, 0x7FFFFFu, 0x400000u}) check_bits(head | m);
                for (int k = 0; k < 64; ++k) check_bits(head | (uint32_t)(rng() & 0x7FFFFFu));
            }
        for (int p = -10; p <= 10; ++p) {
            char text[64];
            for (int k = 1; k <= 9999; ++k) {
                snprintf(text, sizeof text, "%de%d", k, p);
                check_around(strtof(text, nullptr));
            }
            snprintf(text, sizeof text, "999999.5e%d", p);
            const float f = strtof(text, nullptr);
            uint32_t b;
            memcpy(&b, &f, 4);
            for (int d = -40; d <= 40; ++d) check_bits(b + (uint32_t)d);
        }
        for (unsigned long long k = 0; k < n_random; ++k) check_bits((uint32_t)rng());
        printf("checked %llu bad %llu\n", n_checked, n_bad);
        return n_bad ? 1 : 0;
    }
    if (mode == "lines" && argc == 2) {
        std::string line;
        if (!std::getline(std::cin, line)) return 2;
        std::vector<uint32_t> off{0};
        std::string names;
        for (size_t a = 0; a < line.size();) {
            size_t b = line.find(' ', a);
            if (b == std::string::npos) b = line.size();
            const std::vector<uint8_t> nm = unhex(line.substr(a, b - a));
            if (b > a && line.substr(a, b - a) != "-") { names.append(nm.begin(), nm.end()); off.push_back((uint32_t)names.size()); }
            a = b + 1;
        }
        const RefNames refs{off.data(), names.data(), (int32_t)off.size() - 1};
        constexpr size_t kGuard = 64;
        while (std::getline(std::cin, line)) {
            const std::vector<uint8_t> bytes = unhex(line);
            uint8_t* rec = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);      // exactly the record: nothing behind it may be read
            memcpy(rec, bytes.data(), bytes.size());
            uint64_t length = 0;
            const uint32_t st = sam_line_length(rec, bytes.size(), refs, &length);
            uint32_t est = 0;
            bool guards = true;
            std::string hex;
            if (st == kSamOk) {
                uint8_t* buf = (uint8_t*)malloc(length + 2 * kGuard);
                memset(buf, 0xA5, length + 2 * kGuard);
                est = sam_line_emit(rec, bytes.size(), refs, buf + kGuard, length);
                for (size_t k = 0; k < kGuard; ++k) guards = guards && buf[k] == 0xA5 && buf[kGuard + length + k] == 0xA5;
                static const char* digits = "0123456789abcdef";
                hex.reserve(2 * length);
                for (uint64_t k = 0; k < length; ++k) { hex.push_back(digits[buf[kGuard + k] >> 4]); hex.push_back(digits[buf[kGuard + k] & 15]); }
                // a length that is too small must stop the emitter inside the line, not behind it
                if (length > 1) {
                    memset(buf, 0xA5, length + 2 * kGuard);
                    const uint64_t cut = length / 2;
                    const uint32_t cst = sam_line_emit(rec, bytes.size(), refs, buf + kGuard, cut);
                    for (size_t k = 0; k < kGuard; ++k) guards = guards && buf[k] == 0xA5 && buf[kGuard + cut + k] == 0xA5;
                    guards = guards && cst == kSamOverrun;
                }
                free(buf);
            }
            free(rec);
            printf("%u %llu %u %d %s\n", st, (unsigned long long)length, est, guards ? 1 : 0, hex.empty() ? "-" : hex.c_str());
        }
        return 0;
    }
    return 2;
}
