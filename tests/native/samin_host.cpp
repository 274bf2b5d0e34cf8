// samin_host.cpp -- sambamba_amd/csrc/samparse_core.hpp on the CPU (tests/test_samin_core_cpu.py): the statements K15 runs, through the
// very functions the library compiles.
//   samin_host floats SEED N  parse_float against strtof of this machine's C library: every text "%g" can print for a float -- every
//                             significand 1 .. 999999 (without trailing zeros: %g drops them), every decimal exponent -45 .. 38, both
//                             signs, in %g's own spelling --, then N longer literals from the seed: random digit strings of up to 140
//                             digits with random exponents, and the exact decimal expansions of midpoints between neighbouring
//                             floats as they are, with a last digit lowered, and with a non-zero digit behind the 19th, the 117th
//                             and the last place.  Prints the first mismatches and "checked C bad B".
//   samin_host lines          stdin: a line with the hex-encoded reference names ("-": none), then one hex-encoded SAM line per line.
//                             Per line: "status length emit_status guards hexrecord" -- sam_record_length, then sam_record_emit into
//                             a buffer of exactly that length between two guards of 64 bytes (guards: 1 = untouched).  The line lies
//                             in an allocation of exactly its size, so a sanitizer build sees every read behind it.
//   samin_host bins SEED N    record_bin against the bin code of the .bai reader (group_chunks, host_io.hpp): a record filed under
//                             its bin is found by a query for any position it covers, and no deeper bin holds its whole span.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "../../sambamba_amd/csrc/samparse_core.hpp"
#include "../../sambamba_amd/csrc/host_io.hpp"

using namespace sbx::sampc;

static uint64_t rng_state;
static uint64_t rng() {                              // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static std::atomic<unsigned long long> n_checked{0}, n_bad{0};
static void check_text(const std::string& text) {
    const float f = strtof(text.c_str(), nullptr);
    uint32_t want, got = 0xDEADBEEFu;
    memcpy(&want, &f, 4);
    const bool ok = parse_float((const uint8_t*)text.data(), text.size(), &got);
    ++n_checked;
    if ((!ok || got != want) && n_bad++ < 20) printf("mismatch text=%s ok=%d want=%08x got=%08x\n", text.c_str(), (int)ok, want, got);
}

// the exact decimal expansion of m * 2^e (m > 0)
static std::string exact_decimal(uint64_t m, int e) {
    std::vector<uint32_t> d;                          // decimal digits, least significant first
    for (uint64_t x = m; x; x /= 10) d.push_back((uint32_t)(x % 10));
    int point = 0;                                    // digits behind the point
    for (; e > 0; --e) {
        uint32_t carry = 0;
        for (auto& x : d) { const uint32_t t = x * 2 + carry; x = t % 10; carry = t / 10; }
        if (carry) d.push_back(carry);
    }
    for (; e < 0; ++e) {                              // / 2 = * 5 / 10
        uint32_t carry = 0;
        for (auto& x : d) { const uint32_t t = x * 5 + carry; x = t % 10; carry = t / 10; }
        while (carry) { d.push_back(carry % 10); carry /= 10; }
        ++point;
    }
    while ((int)d.size() <= point) d.push_back(0);
    std::string s;
    for (size_t k = d.size(); k-- > 0;) {
        s.push_back((char)('0' + d[k]));
        if ((int)k == point && point) s.push_back('.');
    }
    return s;
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
    if (mode == "floats" && argc == 4) {
        rng_state = strtoull(argv[2], nullptr, 10);
        const unsigned long long n_long = strtoull(argv[3], nullptr, 10);
        // (the exhaustive part is spread over the processors: thread w takes every n_threads-th significand)
        const int n_threads = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
        std::vector<std::thread> pool;
        for (int w = 0; w < n_threads; ++w)
            pool.emplace_back([w, n_threads] {
                char text[64], g[64];
                for (int sig = 1 + w; sig <= 999999; sig += n_threads) {
                    if (sig % 10 == 0) continue;              // (%g never prints a trailing zero of the significand)
                    int nd = 0;
                    for (int x = sig; x; x /= 10) ++nd;
                    for (int x10 = -45; x10 <= 38; ++x10) {
                        // the value sig * 10^(x10 - nd + 1), as %g spells it: through printf of the double nearest to it -- for six
                        // digits the text is the same as for the exact value
                        snprintf(text, sizeof text, "%de%d", sig, x10 - nd + 1);
                        snprintf(g, sizeof g, "%g", strtod(text, nullptr));
                        check_text(g);
                        check_text(std::string("-") + g);
                    }
                }
            });
        for (auto& th : pool) th.join();
        for (unsigned long long k = 0; k < n_long; ++k) {
            // a random digit string with a point somewhere and an exponent that brings it near the float range
            std::string s;
            const int n = 1 + (int)(rng() % 140), point = (int)(rng() % (uint64_t)(n + 1));
            for (int i = 0; i < n; ++i) {
                if (i == point && i) s.push_back('.');
                s.push_back((char)('0' + rng() % 10));
            }
            const int ex = (int)(rng() % 120) - 60 - (point ? point : 0);
            if (rng() & 1) { s += (rng() & 1) ? "e" : "E"; s += std::to_string(ex); }
            check_text(s);
            // a midpoint between two neighbouring floats, exactly; then a hair below and a hair above
            const uint32_t be = (uint32_t)(rng() % 255);                    // biased exponent 0 .. 254
            const uint64_t frac = rng() & 0x7FFFFFu;
            const uint64_t m = (be ? frac | 0x800000u : frac) * 2 + 1;      // 2 * significand + 1
            const int e = (be ? (int)be : 1) - 150 - 1;
            const std::string mid = exact_decimal(m, e);
            check_text(mid);
            for (size_t place : {(size_t)19, (size_t)117, (size_t)1000}) {
                std::string up = mid;
                size_t sig_seen = 0, at = up.size();
                for (size_t i = 0; i < up.size(); ++i) {
                    if (up[i] == '.') continue;
                    if (sig_seen || up[i] != '0') ++sig_seen;
                    if (sig_seen > place) { at = i; break; }
                }
                if (at == up.size()) up += up.find('.') == std::string::npos ? ".0000000001" : "0000000001";      // behind the last place
                else if (up[at] != '9') up[at] = (char)(up[at] + 1);
                else continue;
                check_text(up);
            }
            std::string down = mid;
            size_t last = down.size() - 1;                                   // (the last digit of an exact midpoint is 5)
            if (down[last] >= '1' && down[last] <= '9') { down[last] = (char)(down[last] - 1); down += "9999"; check_text(down); }
        }
        printf("checked %llu bad %llu\n", n_checked.load(), n_bad.load());
        return n_bad ? 1 : 0;
    }
    if (mode == "lines" && argc == 2) {
        std::string row;
        if (!std::getline(std::cin, row)) return 2;
        std::vector<std::string> names;
        for (size_t a = 0; a < row.size();) {
            size_t b = row.find(' ', a);
            if (b == std::string::npos) b = row.size();
            if (b > a && row.substr(a, b - a) != "-") { const std::vector<uint8_t> nm = unhex(row.substr(a, b - a)); names.emplace_back(nm.begin(), nm.end()); }
            a = b + 1;
        }
        std::vector<uint32_t> off{0};
        std::string bytes_of_names;
        for (const std::string& n : names) { bytes_of_names += n; off.push_back((uint32_t)bytes_of_names.size()); }
        const std::vector<uint32_t> slots = ref_table_slots(names);
        const RefTable refs{slots.data(), (uint32_t)slots.size(), off.data(), bytes_of_names.data()};
        constexpr size_t kGuard = 64;
        while (std::getline(std::cin, row)) {
            const std::vector<uint8_t> bytes = unhex(row);
            uint8_t* text = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);      // exactly the line: nothing behind it may be read
            if (!bytes.empty()) memcpy(text, bytes.data(), bytes.size());
            uint64_t length = 0;
            const uint32_t st = sam_record_length(text, bytes.size(), refs, &length);
            uint32_t est = 0;
            bool guards = true;
            std::string hex;
            if (st == kParseOk) {
                uint8_t* buf = (uint8_t*)malloc(length + 2 * kGuard);
                memset(buf, 0xA5, length + 2 * kGuard);
                est = sam_record_emit(text, bytes.size(), refs, buf + kGuard, length);
                for (size_t k = 0; k < kGuard; ++k) guards = guards && buf[k] == 0xA5 && buf[kGuard + length + k] == 0xA5;
                static const char* digits = "0123456789abcdef";
                hex.reserve(2 * length);
                for (uint64_t k = 0; k < length; ++k) { hex.push_back(digits[buf[kGuard + k] >> 4]); hex.push_back(digits[buf[kGuard + k] & 15]); }
                // a length that is too small must stop the emitter inside the record, not behind it
                memset(buf, 0xA5, length + 2 * kGuard);
                const uint64_t cut = length / 2;
                const uint32_t cst = sam_record_emit(text, bytes.size(), refs, buf + kGuard, cut);
                for (size_t k = 0; k < kGuard; ++k) guards = guards && buf[k] == 0xA5 && buf[kGuard + cut + k] == 0xA5;
                guards = guards && cst == kParseOverrun;
                free(buf);
            }
            free(text);
            printf("%u %llu %u %d %s\n", st, (unsigned long long)length, est, guards ? 1 : 0, hex.empty() ? "-" : hex.c_str());
        }
        return 0;
    }
    if (mode == "bins" && argc == 4) {
        rng_state = strtoull(argv[2], nullptr, 10);
        const unsigned long long n = strtoull(argv[3], nullptr, 10);
        auto level_first = [](uint32_t bin) { return bin >= 4681u ? 4681u : bin >= 585u ? 585u : bin >= 73u ? 73u : bin >= 9u ? 9u : bin >= 1u ? 1u : 0u; };
        auto level_shift = [](uint32_t bin) { return bin >= 4681u ? 14u : bin >= 585u ? 17u : bin >= 73u ? 20u : bin >= 9u ? 23u : bin >= 1u ? 26u : 29u; };
        for (unsigned long long k = 0; k < n; ++k) {
            // POS (1-based) and the reference span of the CIGAR, inside the 2^29 positions the binning scheme covers
            const uint32_t shape = (uint32_t)(rng() % 4);
            uint32_t pos = 1u + (uint32_t)(rng() % ((1u << 29) - 2u));
            if (shape == 0) pos = (pos & ~0x3FFFu) + (uint32_t)(rng() % 3);                    // at a 16 KiB boundary
            if (pos == 0) pos = 1;
            uint32_t span = shape == 1 ? 0u : shape == 2 ? (uint32_t)(rng() % 300) : (uint32_t)(rng() % (1u << (rng() % 29)));
            if ((uint64_t)pos + span > (1ull << 29)) span = (1u << 29) - pos;
            const uint32_t bin = record_bin(pos, span);
            ++n_checked;
            const uint32_t beg = pos - 1u, end = span ? beg + span : beg + 1u;                  // 0-based, half open
            // the bin holds the whole span, and no bin one level deeper does
            const uint32_t sh = level_shift(bin), first = level_first(bin);
            bool good = bin == 0u ? true : (bin - first == beg >> sh && bin - first == (end - 1u) >> sh);
            if (bin < 4681u) { const uint32_t deeper = sh - 3u; good = good && (beg >> deeper != (end - 1u) >> deeper); }
            // the .bai reader asks for this bin whatever covered position the query names
            sbx::BaiIndex bai;
            bai.refs.resize(1);
            bai.refs[0].bins.push_back(sbx::BaiBin{bin, {sbx::BaiChunk{100, 200}}});
            for (uint32_t q : {beg, end - 1u, beg + (end - beg) / 2u}) {
                const std::vector<sbx::BaiChunk> found = sbx::group_chunks(bai, {sbx_region{0u, q, q + 1u}});
                good = good && found.size() == 1 && found[0].beg == 100 && found[0].end == 200;
            }
            if (!good && n_bad++ < 20) printf("mismatch pos=%u span=%u bin=%u\n", pos, span, bin);
        }
        // POS 0: the interval [-1, 0) lies in front of the first window
        ++n_checked;
        if (record_bin(0u, 0u) != 4680u && n_bad++ < 20) printf("mismatch pos=0 bin=%u\n", record_bin(0u, 0u));
        printf("checked %llu bad %llu\n", n_checked.load(), n_bad.load());
        return n_bad ? 1 : 0;
    }
    return 2;
}
