// namesort_host.cpp -- sambamba_amd/csrc/namesort_core.hpp on the CPU (tests/test_namesort_core_cpu.py): the statements K14 runs,
// through the very functions the library compiles.
//   namesort_host known           the nine known answers of mixedStrCompare (BioD read.d:1573-1581) and a few of name_less.
//   namesort_host exhaustive      every string of length 0..4 over {'0','1','9','/',':','a','~'} (2801 strings, every ordered pair):
//                                 the sign of the order of the encoded, zero-padded words equals the sign of the comparator, for
//                                 both orders, and two keys are equal only for identical names.
//   namesort_host random SEED N   the same over N seeded names of up to 254 bytes (digit runs of 1, 8, 9 and 254 digits, runs of
//                                 zeros, names that are prefixes of others), plus the sinks: measured length = written length, the
//                                 guard words behind the bounded writer stay intact (also when the capacity is too small), no key
//                                 byte is zero, no key has more than kMaxKeyWords words.
//   namesort_host hi              stdin: one hex-encoded aux area per line ("-": empty).  Per line "ok hi": find_hi over an
//                                 allocation of exactly that size, so a sanitizer build sees every read behind it.
//   namesort_host words ORDER     stdin: one name per line.  Per line the words of its key (decimal), as key_words and key_emit give
//                                 them for ORDER (1 lexicographic, 2 natural).
// The first three modes print "checked C bad B" last and exits with 1 when B != 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/namesort_core.hpp"

using namespace sbx::nsc;

static uint64_t rng_state;
static uint64_t rng() {                              // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static unsigned long long n_checked = 0, n_bad = 0;
static void fail(const char* what, const std::string& a, const std::string& b) {
    if (n_bad++ < 20) printf("FAIL %s: \"%s\" \"%s\"\n", what, a.c_str(), b.c_str());
}
static int sign(int v) { return v < 0 ? -1 : v > 0 ? 1 : 0; }
static const uint8_t* u8(const std::string& s) { return (const uint8_t*)s.data(); }

static int cmp_names(const std::string& a, const std::string& b, uint32_t order) {
    if (order == kOrderNatural) return sign(mixed_str_compare(u8(a), (uint32_t)a.size(), u8(b), (uint32_t)b.size()));
    return name_less(u8(a), (uint32_t)a.size(), u8(b), (uint32_t)b.size()) ? -1 : name_less(u8(b), (uint32_t)b.size(), u8(a), (uint32_t)a.size()) ? 1 : 0;
}

// the order the sort sees: word by word as unsigned numbers, a missing word is 0
static int cmp_keys(const std::vector<uint64_t>& a, const std::vector<uint64_t>& b) {
    const size_t m = a.size() > b.size() ? a.size() : b.size();
    for (size_t k = 0; k < m; ++k) {
        const uint64_t x = k < a.size() ? a[k] : 0, y = k < b.size() ? b[k] : 0;
        if (x != y) return x < y ? -1 : 1;
    }
    return 0;
}

constexpr uint32_t kGuardWords = 8;
constexpr uint64_t kGuard = 0xA5A5A5A5A5A5A5A5ull;

// the key of a name through both sinks, with everything the sinks promise checked on the way
static std::vector<uint64_t> checked_key(const std::string& name, uint32_t order) {
    const uint32_t n = (uint32_t)name.size();
    const uint32_t bytes = key_bytes(u8(name), n, order), words = key_words(u8(name), n, order);
    ++n_checked;
    if (words != (bytes + 7) / 8 || words > kMaxKeyWords) fail("measured length", name, "");
    uint64_t* buf = (uint64_t*)malloc((words + kGuardWords) * 8);
    for (uint32_t k = 0; k < words + kGuardWords; ++k) buf[k] = kGuard;
    uint32_t got = 0;
    if (!key_emit(u8(name), n, order, buf, words, &got) || got != words) fail("written length", name, "");
    for (uint32_t k = 0; k < kGuardWords; ++k) if (buf[words + k] != kGuard) fail("guard", name, "");
    std::vector<uint64_t> key(buf, buf + words);
    for (uint32_t k = 0; k < 8 * words; ++k) {
        const uint8_t b = (uint8_t)(key[k / 8] >> (56 - 8 * (k % 8)));
        if ((k < bytes) != (b != 0)) fail("zero key byte or non-zero padding", name, "");
    }
    if (order == kOrderLex) {
        bool same = bytes == n;
        for (uint32_t k = 0; same && k < n; ++k) same = (uint8_t)(key[k / 8] >> (56 - 8 * (k % 8))) == (uint8_t)name[k];
        if (!same) fail("lexicographic key is not the name", name, "");
    }
    // a capacity that is too small stops the writer inside it
    if (words > 1) {
        const uint32_t cut = words / 2;
        for (uint32_t k = 0; k < words + kGuardWords; ++k) buf[k] = kGuard;
        if (key_emit(u8(name), n, order, buf, cut, &got)) fail("overrun not reported", name, "");
        for (uint32_t k = cut; k < words + kGuardWords; ++k) if (buf[k] != kGuard) fail("guard behind a short buffer", name, "");
        for (uint32_t k = 0; k < cut; ++k) if (buf[k] != key[k]) fail("words in front of the cut", name, "");
    }
    free(buf);
    return key;
}

static void check_all_pairs(const std::vector<std::string>& names) {
    for (uint32_t order : {(uint32_t)kOrderLex, (uint32_t)kOrderNatural}) {
        std::vector<std::vector<uint64_t>> keys;
        keys.reserve(names.size());
        for (const std::string& s : names) keys.push_back(checked_key(s, order));
        for (size_t i = 0; i < names.size(); ++i)
            for (size_t j = 0; j < names.size(); ++j) {
                const int c = cmp_names(names[i], names[j], order), k = cmp_keys(keys[i], keys[j]);
                ++n_checked;
                if (c != k) fail(order == kOrderLex ? "order -n" : "order -N", names[i], names[j]);
                if ((k == 0) != (names[i] == names[j])) fail("equal keys", names[i], names[j]);
            }
    }
}

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((uint8_t)(v(h[k]) << 4 | v(h[k + 1])));
    return out;
}

static int finish() {
    printf("checked %llu bad %llu\n", n_checked, n_bad);
    return n_bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "known") {
        struct { const char *a, *b; int want; } mixed[] = {
            {"BC0123", "BC01234", -1}, {"BC0123", "BC0123Z", -1}, {"BC01234", "BC01234", 0}, {"BC0123DEF45", "BC01234DEF45", -1},
            {"BC01236DEF45", "BC01234DEF45", 1}, {"BC012", "BC0012", -1}, {"BC0012DE0034", "BC0012DE34", 1}, {"BC12DE0034", "BC012DE34", -1},
            {"1235", "1234", 1}};
        for (auto& m : mixed) {
            ++n_checked;
            if (cmp_names(m.a, m.b, kOrderNatural) != m.want || cmp_names(m.b, m.a, kOrderNatural) != -m.want) fail("known answer -N", m.a, m.b);
        }
        struct { const char *a, *b; int want; } lex[] = {{"", "", 0}, {"", "a", -1}, {"a", "ab", -1}, {"ab", "b", -1}, {"a10", "a9", -1},
                                                          {"a~", "a\x7f", -1}, {"B", "a", -1}, {"abc", "abc", 0}};
        for (auto& m : lex) {
            ++n_checked;
            if (cmp_names(m.a, m.b, kOrderLex) != m.want || cmp_names(m.b, m.a, kOrderLex) != -m.want) fail("known answer -n", m.a, m.b);
        }
        // the -M word orders (HI, flag) as signed HI, then flag
        const int32_t his[] = {INT32_MIN, -70000, -1, 0, 1, 255, 65536, INT32_MAX};
        const uint32_t flags[] = {0, 0x40, 0x80, 0xFFFF};
        uint64_t last = 0;
        bool first = true;
        for (int32_t h : his)
            for (uint32_t f : flags) {
                const uint64_t w = mate_word(h, f);
                ++n_checked;
                if (!first && w <= last) fail("mate_word is not increasing", std::to_string(h), std::to_string(f));
                if (w >> 48) fail("mate_word has more than 48 bits", std::to_string(h), std::to_string(f));
                last = w;
                first = false;
            }
        return finish();
    }
    if (mode == "exhaustive") {
        const char alphabet[] = {'0', '1', '9', '/', ':', 'a', '~'};
        std::vector<std::string> names{""};
        for (size_t lo = 0, len = 1; len <= 4; ++len) {
            const size_t hi = names.size();
            for (size_t k = lo; k < hi; ++k)
                for (char c : alphabet) names.push_back(names[k] + c);
            lo = hi;
        }
        if (names.size() != 2801) fail("2801 strings", std::to_string(names.size()), "");
        check_all_pairs(names);
        return finish();
    }
    if (mode == "random" && argc == 4) {
        rng_state = strtoull(argv[2], nullptr, 10);
        const size_t n = (size_t)strtoull(argv[3], nullptr, 10);
        std::vector<std::string> names;
        auto digits = [&](size_t len, bool zeros_only) {
            std::string s;
            const size_t nz = zeros_only ? len : rng() % 3 == 0 ? rng() % (len + 1) : 0;
            for (size_t k = 0; k < len; ++k) s.push_back(k < nz ? '0' : (char)('0' + rng() % (rng() % 2 ? 10 : 2)));
            return s;
        };
        // the lengths the issue names, as whole names and inside one
        for (size_t len : {1u, 8u, 9u, 254u}) {
            for (int rep = 0; rep < 3; ++rep) names.push_back(digits(len, false));
            names.push_back(digits(len, true));
            names.push_back(std::string(len, '9'));
            if (len + 2 <= kMaxNameLen) { names.push_back("r" + digits(len, false) + "x"); names.push_back("r" + digits(len, true) + "x"); }
        }
        names.push_back(std::string(253, '0') + "1");
        names.push_back(std::string(253, '0'));
        { std::string s; for (int k = 0; k < 127; ++k) s += "1a"; names.push_back(s); }      // the longest key: 635 bytes
        { std::string s; for (int k = 0; k < 127; ++k) s += "a0"; names.push_back(s); }
        static const char* const pieces[] = {"a", "b", ":", "/", "~", "!", "\x7f", "\x01", "read", "HWI-ST", "_"};
        while (names.size() < n) {
            std::string s;
            if (rng() % 4 == 0 && !names.empty()) s = names[rng() % names.size()];           // extend (or repeat) an earlier name
            const size_t want = rng() % 6 == 0 ? rng() % (kMaxNameLen + 1) : rng() % 24;
            while (s.size() < want) {
                if (rng() % 2) s += pieces[rng() % (sizeof pieces / sizeof *pieces)];
                else { static const size_t lens[] = {1, 1, 2, 3, 8, 9, 12}; s += digits(lens[rng() % 7], rng() % 5 == 0); }
            }
            if (s.size() > kMaxNameLen) s.resize(kMaxNameLen);
            names.push_back(s);
            if (rng() % 3 == 0 && !s.empty()) names.push_back(s.substr(0, rng() % s.size()));  // a proper prefix of it
        }
        check_all_pairs(names);
        return finish();
    }
    if (mode == "words" && argc == 3) {
        const uint32_t order = (uint32_t)atoi(argv[2]);
        std::string line;
        while (std::getline(std::cin, line)) {
            const uint32_t words = key_words(u8(line), (uint32_t)line.size(), order);
            std::vector<uint64_t> key(words + 1);
            uint32_t got = 0;
            if (!key_emit(u8(line), (uint32_t)line.size(), order, key.data(), words, &got) || got != words) return 1;
            for (uint32_t k = 0; k < words; ++k) printf("%s%llu", k ? " " : "", (unsigned long long)key[k]);
            printf("\n");
        }
        return 0;
    }
    if (mode == "hi" && argc == 2) {
        std::string line;
        while (std::getline(std::cin, line)) {
            const std::vector<uint8_t> bytes = unhex(line);
            uint8_t* aux = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);               // exactly the aux area
            if (!bytes.empty()) memcpy(aux, bytes.data(), bytes.size());
            int32_t hi = 12345;
            const bool ok = find_hi(aux, 0, bytes.size(), &hi);
            free(aux);
            printf("%d %d\n", ok ? 1 : 0, hi);
            ++n_checked;
        }
        return 0;
    }
    return 2;
}
