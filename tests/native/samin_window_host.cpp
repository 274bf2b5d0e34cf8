// samin_window_host.cpp -- sampc::WindowSink / sam_record_emit_window of sambamba_amd/csrc/samparse_core.hpp on the CPU
// (tests/test_samin_window_cpu.py): the statements K15d runs for a record that straddles a window edge, through the very functions
// the library compiles, against what sam_record_emit writes for the same line.
//   samin_window_host   stdin: a line with the hex-encoded reference names ("-": none), then per SAM line two lines: the line
//                       hex-encoded, and its cuts -- "all" (every c in [0, length]) or decimal numbers.  The record lies at `kOff` of an
//                       imagined output stream.  For every cut c:
//                         [0, c) and [c, length)  each window into a buffer of exactly its size between two guards of 64 bytes: the bytes
//                                                 reported are c and length - c, the two parts are the record's, the status is kParseOk;
//                         [c, c + 8)              the same, the window clips the record on both sides (or reaches past its end: the
//                                                 bytes behind the record stay as they were);
//                         one byte short          [c, c + 8) with the measured length lowered by one: kParseOverrun, and no byte outside
//                                                 the clip changes.
//                       No guard byte may change.  Per SAM line: "status length cuts failures first_failure".
//                       The line lies in an allocation of exactly its size, so a sanitizer build sees every read behind it.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../sambamba_amd/csrc/samparse_core.hpp"

using namespace sbx::sampc;

static constexpr size_t kGuard = 64;
static constexpr uint8_t kFillByte = 0xA5;
static constexpr uint64_t kOff = 5000000011ull;         // (past 2^32, odd: the place of the record in the stream)

static std::vector<uint8_t> unhex(const std::string& h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; };
    out.reserve(h.size() / 2);
    for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((uint8_t)(v(h[k]) << 4 | v(h[k + 1])));
    return out;
}

struct Line {
    const uint8_t* text;
    uint64_t n;
    const RefTable* refs;
    const uint8_t* rec;         // what sam_record_emit wrote
    uint64_t length;
};

// One window [a, b) of the record's own bytes (b may lie behind the record), the record measured as `length`.  `buf` has room for
// b - a bytes between its guards.  Returns "" or what is wrong.
static std::string one_window(const Line& l, uint64_t a, uint64_t b, uint64_t length, std::vector<uint8_t>& buf) {
    const uint64_t span = b - a;
    buf.assign(span + 2 * kGuard, kFillByte);
    uint64_t wrote = ~0ull;
    const uint32_t st = sam_record_emit_window(l.text, l.n, *l.refs, kOff, length, buf.data() + kGuard,kOff + a, kOff + b, &wrote);
    for (size_t k = 0; k < kGuard; ++k)
        if (buf[k] != kFillByte || buf[kGuard + span + k] != kFillByte) return "a guard byte changed";
    const uint64_t inside = a < length ? (b < length ? b : length) - a : 0;      // bytes of [a, b) that belong to the record
    for (uint64_t k = inside; k < span; ++k)
        if (buf[kGuard + k] != kFillByte) return "a byte behind the record changed";
    if (length != l.length) {                           // measured one byte short: nothing to compare but the verdict
        if (st != kParseOverrun) return "a record measured too short is not an overrun";
        if (wrote > inside) return "more bytes reported than the clip holds";
        return "";
    }
    if (st != kParseOk) return "status " + std::to_string(st);
    if (wrote != inside) return "reported " + std::to_string(wrote) + " bytes, not " + std::to_string(inside);
    if (inside && memcmp(buf.data() + kGuard, l.rec + a, inside) != 0) return "the bytes differ from sam_record_emit's";
    return "";
}

static std::string one_cut(const Line& l, uint64_t c, std::vector<uint8_t>& buf) {
    std::string e;
    if (!(e = one_window(l, 0, c, l.length, buf)).empty()) return "[0, c): " + e;
    if (!(e = one_window(l, c, l.length, l.length, buf)).empty()) return "[c, length): " + e;
    if (!(e = one_window(l, c, c + 8, l.length, buf)).empty()) return "[c, c + 8): " + e;
    if (!(e = one_window(l, c, c + 8, l.length - 1, buf)).empty()) return "one byte short: " + e;
    return "";
}

int main() {
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
    const unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));

    std::string cut_row;
    while (std::getline(std::cin, row) && std::getline(std::cin, cut_row)) {
        const std::vector<uint8_t> bytes = unhex(row);
        uint8_t* text = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);          // exactly the line: nothing behind it may be read
        if (!bytes.empty()) memcpy(text, bytes.data(), bytes.size());
        uint64_t length = 0;
        const uint32_t st = sam_record_length(text, bytes.size(), refs, &length);
        if (st != kParseOk) { printf("%u 0 0 0 -\n", st); free(text); continue; }
        std::vector<uint8_t> rec(length);
        if (sam_record_emit(text, bytes.size(), refs, rec.data(), length) != kParseOk) { printf("9 0 0 0 -\n"); free(text); continue; }
        std::vector<uint64_t> cuts;
        if (cut_row == "all") for (uint64_t c = 0; c <= length; ++c) cuts.push_back(c);
        else {
            const char* p = cut_row.c_str();
            char* end = nullptr;
            for (;;) {
                const unsigned long long c = strtoull(p, &end, 10);
                if (end == p) break;
                if (c <= length) cuts.push_back(c);
                p = end;
            }
        }
        const Line l{text, bytes.size(), &refs, rec.data(), length};
        std::atomic<size_t> next{0};
        std::atomic<unsigned long long> failures{0};
        std::mutex m;
        std::string first;
        std::vector<std::thread> pool;
        for (unsigned w = 0; w < n_threads; ++w)
            pool.emplace_back([&] {
                std::vector<uint8_t> buf;
                for (size_t k; (k = next++) < cuts.size();) {
                    const std::string e = one_cut(l, cuts[k], buf);
                    if (e.empty()) continue;
                    ++failures;
                    std::lock_guard<std::mutex> g(m);
                    if (first.empty()) first = "c=" + std::to_string(cuts[k]) + ":" + e;
                }
            });
        for (auto& th : pool) th.join();
        for (char& ch : first) if (ch == ' ') ch = '_';
        printf("0 %llu %zu %llu %s\n", (unsigned long long)length, cuts.size(), failures.load(), first.empty() ? "-" : first.c_str());
        free(text);
    }
    return 0;
}
