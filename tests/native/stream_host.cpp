// stream_host.cpp -- the arithmetic of K21 (sambamba_amd/csrc/stream_core.hpp) on the CPU: what one record puts into one staging
// window of the output stream, against a byte-wise restatement with guard bytes around the window.
//
//   stream_host plan W      for a window of W bytes at several places of the stream: every combination of record start and length
//                           relative to [w0, w1) -- before, cut at the front, inside, cut at the back, spanning the whole window,
//                           behind it, and every start within 20 bytes of either edge --, with and without the bin patch (so byte 14
//                           is the last byte of the window and byte 15 the first of the next in some of them).  The plan is applied
//                           byte by byte; no byte outside the window may be written, no byte of it twice, every byte that belongs
//                           exactly once and with the right value, and wrote() must be their number.  Prints "cases N patched_split M"
//                           (M: cases where exactly one of the two bin bytes fell into the window).
//   stream_host stream W H  a stream of H header bytes and a fixed list of records written through consecutive windows of W bytes
//                           with window_record_bytes as the check of every window: prints the stream to stdout (the test compares
//                           it with its own) and "windows K" to stderr.
// Exit 0: all as stated; 1: a difference (said on stderr); 2: usage.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/stream_core.hpp"

using namespace sbx;

namespace {

constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0xA5, kUnset = 0x5A;

uint8_t rec_byte(uint64_t rec, uint64_t j) { return (uint8_t)((rec * 131 + j * 7 + 3) % 127); }

// the plan applied the way K21 applies it, counting the writes per byte of the buffer (guards included)
void apply(const streamc::PackPlan& p, const std::vector<uint8_t>& rec, std::vector<uint8_t>& buf, std::vector<uint32_t>& writes) {
    for (uint32_t k = 0; k < p.n_spans; ++k)
        for (uint64_t b = 0; b < p.span[k].len; ++b) {
            const size_t at = kGuard + (size_t)(p.span[k].dst + b);
            buf.at(at) = rec.at((size_t)(p.span[k].src + b));
            ++writes.at(at);
        }
    for (uint32_t k = 0; k < p.n_bytes; ++k) {
        const size_t at = kGuard + (size_t)p.byte_dst[k];
        buf.at(at) = p.byte_val[k];
        ++writes.at(at);
    }
}

bool one_case(uint64_t dest, uint64_t len, uint64_t w0, uint64_t w1, uint32_t bin, uint64_t id, bool* split) {
    std::vector<uint8_t> rec((size_t)len);
    for (uint64_t j = 0; j < len; ++j) rec[(size_t)j] = rec_byte(id, j);
    const size_t W = (size_t)(w1 - w0);
    std::vector<uint8_t> got(W + 2 * kGuard, kGuardByte), want(W + 2 * kGuard, kGuardByte);
    std::fill(got.begin() + kGuard, got.begin() + kGuard + W, kUnset);
    std::fill(want.begin() + kGuard, want.begin() + kGuard + W, kUnset);
    std::vector<uint32_t> writes(got.size(), 0);
    // the restatement: byte j of the record lies at byte dest + j of the stream
    uint64_t belong = 0;
    uint32_t bin_bytes_in = 0;
    for (uint64_t j = 0; j < len; ++j) {
        const uint64_t at = dest + j;
        if (at < w0 || at >= w1) continue;
        uint8_t v = rec[(size_t)j];
        if (bin != streamc::kNoPatch && j == 14) { v = (uint8_t)bin; ++bin_bytes_in; }
        if (bin != streamc::kNoPatch && j == 15) { v = (uint8_t)(bin >> 8); ++bin_bytes_in; }
        want[kGuard + (size_t)(at - w0)] = v;
        ++belong;
    }
    *split = bin_bytes_in == 1;
    streamc::PackPlan p;
    streamc::plan_record(dest, len, w0, w1, bin, &p);
    for (uint32_t k = 0; k < p.n_spans; ++k)
        if (p.span[k].len == 0 || p.span[k].dst + p.span[k].len > W || p.span[k].src + p.span[k].len > len) {
            fprintf(stderr, "span outside: dest=%llu len=%llu w=[%llu,%llu) bin=%x\n", (unsigned long long)dest, (unsigned long long)len,
                    (unsigned long long)w0, (unsigned long long)w1, bin);
            return false;
        }
    for (uint32_t k = 0; k < p.n_bytes; ++k)
        if (p.byte_dst[k] >= W) { fprintf(stderr, "patch byte outside\n"); return false; }
    apply(p, rec, got, writes);
    bool ok = got == want && p.wrote() == belong;
    for (size_t k = 0; k < writes.size(); ++k) {
        const bool inside = k >= kGuard && k < kGuard + W;
        if (writes[k] > 1 || (!inside && writes[k])) ok = false;
    }
    uint64_t written = 0;
    for (uint32_t w : writes) written += w;
    if (written != belong) ok = false;
    if (!ok)
        fprintf(stderr, "difference: dest=%llu len=%llu w=[%llu,%llu) bin=%x wrote=%llu belong=%llu\n", (unsigned long long)dest,
                (unsigned long long)len, (unsigned long long)w0, (unsigned long long)w1, bin, (unsigned long long)p.wrote(),
                (unsigned long long)belong);
    return ok;
}

int run_plan(uint64_t W) {
    uint64_t cases = 0, n_split = 0, id = 0;
    const uint64_t w0s[] = {0, W, 1000 * W};
    for (uint64_t w0 : w0s) {
        const uint64_t w1 = w0 + W;
        std::vector<uint64_t> lens = {36, 37, 52, 100, W, W + 1, W + 36, 2 * W + 40, 3 * W + 36};
        for (uint64_t len : lens) {
            if (len < 36) continue;
            // starts: far before, every start whose record touches an edge within 20 bytes, inside, far behind
            std::vector<int64_t> starts;
            const int64_t a = (int64_t)w0, b = (int64_t)w1, L = (int64_t)len;
            starts.push_back(a - L - 50);                                       // before
            for (int64_t d = -20; d <= 20; ++d) {
                starts.push_back(a - L + d);                                    // its end around w0
                starts.push_back(a + d);                                        // its start around w0
                starts.push_back(b - L + d);                                    // its end around w1
                starts.push_back(b + d);                                        // its start around w1
            }
            starts.push_back(a + (int64_t)(W / 2));                             // inside (or cut at the back)
            starts.push_back(a - L / 2);                                        // cut at the front (or spanning)
            starts.push_back(b + 100);                                          // behind
            for (int64_t st : starts) {
                if (st < 0) continue;
                for (uint32_t bin : {streamc::kNoPatch, 0x1249u, 0xFF00u, 0u}) {
                    bool split = false;
                    if (!one_case((uint64_t)st, len, w0, w1, bin, id++, &split)) return 1;
                    ++cases;
                    n_split += split;
                }
            }
        }
        // byte 14 the last byte of the window, byte 15 the first of the next -- and the window behind it, which gets byte 15 only
        for (uint64_t w : {w0, w1}) {
            if (w1 < 15) continue;
            bool split = false;
            if (!one_case(w1 - 15, 48, w, w + W, 0xBEEFu, id++, &split)) return 1;
            ++cases;
            n_split += split;
        }
    }
    printf("cases %llu patched_split %llu\n", (unsigned long long)cases, (unsigned long long)n_split);
    return 0;
}

int run_stream(uint64_t W, uint64_t H) {
    const uint64_t lens[] = {36, 40, 200, 3 * W + 36, 36, 77, W, 36, 2 * W + 1, 50};
    const size_t n = sizeof lens / sizeof lens[0];
    std::vector<uint64_t> dest(n);
    uint64_t total = H;
    for (size_t i = 0; i < n; ++i) { dest[i] = total; total += lens[i]; }
    std::vector<uint8_t> stream;
    uint64_t windows = 0;
    for (uint64_t w0 = 0; w0 < total; w0 += W, ++windows) {
        const uint64_t w1 = w0 + W, end = total < w1 ? total : w1;
        std::vector<uint8_t> buf((size_t)W + 2 * kGuard, kGuardByte);
        std::vector<uint32_t> writes(buf.size(), 0);
        for (uint64_t at = w0; at < end && at < H; ++at) buf[kGuard + (size_t)(at - w0)] = (uint8_t)(0x80 | (at % 127));
        uint64_t wrote = 0;
        for (size_t i = 0; i < n; ++i) {
            std::vector<uint8_t> rec((size_t)lens[i]);
            for (uint64_t j = 0; j < lens[i]; ++j) rec[(size_t)j] = rec_byte(i, j);
            streamc::PackPlan p;
            streamc::plan_record(dest[i], lens[i], w0, w1, i % 2 ? 0x1234u + (uint32_t)i : streamc::kNoPatch, &p);
            apply(p, rec, buf, writes);
            wrote += p.wrote();
        }
        if (wrote != streamc::window_record_bytes(w0, w1, H, total)) {
            fprintf(stderr, "window [%llu, %llu): %llu bytes arrived, %llu belong\n", (unsigned long long)w0, (unsigned long long)w1,
                    (unsigned long long)wrote, (unsigned long long)streamc::window_record_bytes(w0, w1, H, total));
            return 1;
        }
        for (size_t k = 0; k < buf.size(); ++k) {
            const bool outside = k < kGuard || k >= kGuard + (size_t)(end - w0);      // the guards, and what lies behind the stream's end
            if (writes[k] > 1 || (outside && (writes[k] || buf[k] != kGuardByte))) {
                fprintf(stderr, "window [%llu, %llu): byte %zu written %u times\n", (unsigned long long)w0, (unsigned long long)w1, k, writes[k]);
                return 1;
            }
        }
        stream.insert(stream.end(), buf.begin() + kGuard, buf.begin() + kGuard + (size_t)(end - w0));
    }
    fwrite(stream.data(), 1, stream.size(), stdout);
    fprintf(stderr, "windows %llu\n", (unsigned long long)windows);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "plan")) return run_plan(strtoull(argv[2], nullptr, 10));
    if (argc >= 4 && !strcmp(argv[1], "stream")) return run_stream(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    fprintf(stderr, "usage: stream_host plan W | stream W H\n");
    return 2;
}
