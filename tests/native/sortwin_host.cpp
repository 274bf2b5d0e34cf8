// sortwin_host.cpp -- the window arithmetic of the windowed sort (sambamba_amd/csrc/sort_core.hpp) on the CPU
// (tests/test_sort_windows_core_cpu.py), through the very functions the library and K9d compile.  Built with -fsanitize=address,undefined.
//   sortwin_host plan PIECE MAXPIECES MAXWINDOW   for every total in {k * PIECE - 1, k * PIECE, k * PIECE + 1 : k = 0 .. MAXPIECES} and every
//                               window size of 1 .. MAXWINDOW pieces -- given as w * PIECE, as w * PIECE - 1 and as (w - 1) * PIECE + 1 bytes,
//                               which all round up to w pieces -- one line "total window_bytes : w0 w1 w0 w1 ..." (plan_windows)
//   sortwin_host clip HLEN PIECE WINDOW BATCH     lines "len rank" on stdin, one per record in file order (rank: its place in the sorted
//                               order) -> the stream of HLEN header bytes + the records in sorted order, assembled window by window the
//                               way the windowed sort does it: dest of every record, the span of every batch of BATCH records, the
//                               batches span_meets_window admits, clip_to_piece of [dest, dest + len) for each of their records.
//                               stdout: the windows one behind the other.  stderr per window: "window k w0 w1 unwritten twice outside
//                               runs skipped whole" -- bytes of [0, w1 - w0) written never / more than once, writes outside it, batches
//                               run and skipped, and whether window_refusal accepts the bytes counted.
//   sortwin_host refusal W0 W1 HLEN BYTES MISMATCHES [sort|markdup]   -> the text of window_refusal in the command's words (sort when
//                               not given) on stdout; exit status 3 when there is one
//   sortwin_host words sort|markdup              -> the two other refusals in the command's words, one per line: batch_refusal, and
//                               windows_do_not_fit for 1000 bytes needed, 10 free and the command's own window_needs
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/sort_core.hpp"

using namespace sbx::sortc;

static uint8_t header_byte(uint64_t j) { return (uint8_t)(0x80 | (j % 127)); }
static uint8_t record_byte(uint64_t i, uint64_t j) { return (uint8_t)((i * 131 + j * 7 + 3) % 127); }

static int plan(uint64_t piece, uint64_t max_pieces, uint64_t max_window) {
    if (!piece) return 2;
    for (uint64_t k = 0; k <= max_pieces; ++k)
        for (int d = -1; d <= 1; ++d) {
            if (k == 0 && d < 0) continue;
            const uint64_t total = k * piece + d;
            for (uint64_t w = 1; w <= max_window; ++w)
                for (uint64_t wb : {w * piece, w * piece - 1, (w - 1) * piece + 1}) {
                    if (wb == 0 || (wb - 1) / piece + 1 != w) continue;          // (piece 1: the three coincide or leave the size)
                    printf("%llu %llu :", (unsigned long long)total, (unsigned long long)wb);
                    for (const Window& x : plan_windows(total, piece, wb)) printf(" %llu %llu", (unsigned long long)x.w0, (unsigned long long)x.w1);
                    printf("\n");
                }
        }
    return 0;
}

static int clip(uint64_t hlen, uint64_t piece, uint64_t window_bytes, uint64_t batch) {
    if (!piece || !batch) return 2;
    std::vector<uint64_t> len, rank;
    unsigned long long l, r;
    while (scanf("%llu %llu", &l, &r) == 2) { len.push_back(l); rank.push_back(r); }
    const uint64_t n = len.size();
    std::vector<uint64_t> at(n), dest(n);            // at[rank] = record
    for (uint64_t i = 0; i < n; ++i) { if (rank[i] >= n) return 2; at[rank[i]] = i; }
    uint64_t total = hlen;
    for (uint64_t q = 0; q < n; ++q) { dest[at[q]] = total; total += len[at[q]]; }
    // the spans of the batches (K9d-2)
    const uint64_t nb = (n + batch - 1) / batch;
    std::vector<uint64_t> lo(nb, ~0ull), hi(nb, 0);
    for (uint64_t i = 0; i < n; ++i) { lo[i / batch] = std::min(lo[i / batch], dest[i]); hi[i / batch] = std::max(hi[i / batch], dest[i] + len[i]); }
    const uint64_t span = window_span(piece, window_bytes), guard = 64;
    std::vector<uint8_t> buf(span + 2 * guard);
    std::vector<uint32_t> cnt(span + 2 * guard);
    uint64_t k = 0;
    for (const Window& w : plan_windows(total, piece, window_bytes)) {
        std::fill(buf.begin(), buf.end(), (uint8_t)0xEE);
        std::fill(cnt.begin(), cnt.end(), 0u);
        uint64_t outside = 0, runs = 0, skipped = 0, record_bytes = 0;
        auto put = [&](uint64_t a, uint8_t v) {      // byte a of the window; unsigned: below zero shows as huge
            if (a >= w.w1 - w.w0) ++outside;
            const uint64_t g = a + guard;
            if (g < buf.size()) { buf[g] = v; ++cnt[g]; }
        };
        PieceClip c;
        if (clip_to_piece(0, hlen, w.w0, w.w1, &c))
            for (uint64_t b = 0; b < c.len; ++b) put(c.dst + b, header_byte(c.src + b));
        for (uint64_t bt = 0; bt < nb; ++bt) {
            if (!span_meets_window(lo[bt], hi[bt], w.w0, w.w1)) { ++skipped; continue; }
            ++runs;
            for (uint64_t i = bt * batch; i < std::min(n, (bt + 1) * batch); ++i) {
                if (!clip_to_piece(dest[i], dest[i] + len[i], w.w0, w.w1, &c)) continue;
                for (uint64_t b = 0; b < c.len; ++b) put(c.dst + b, record_byte(i, c.src + b));
                record_bytes += c.len;
            }
        }
        uint64_t unwritten = 0, twice = 0;
        for (uint64_t j = 0; j < w.w1 - w.w0; ++j) { unwritten += cnt[guard + j] == 0; twice += cnt[guard + j] > 1; }
        fprintf(stderr, "window %llu %llu %llu %llu %llu %llu %llu %llu %d\n", (unsigned long long)k, (unsigned long long)w.w0, (unsigned long long)w.w1,
                (unsigned long long)unwritten, (unsigned long long)twice, (unsigned long long)outside, (unsigned long long)runs,
                (unsigned long long)skipped, window_refusal(w.w0, w.w1, hlen, record_bytes, 0).empty() ? 1 : 0);
        fwrite(buf.data() + guard, 1, (size_t)(w.w1 - w.w0), stdout);
        ++k;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    auto num = [&](int k) { return strtoull(argv[k], nullptr, 10); };
    if (mode == "plan" && argc == 5) return plan(num(2), num(3), num(4));
    if (mode == "clip" && argc == 6) return clip(num(2), num(3), num(4), num(5));
    auto words = [&](int k) -> const WindowWords* {
        if (k >= argc || std::string(argv[k]) == "sort") return &kSortWindowWords;
        return std::string(argv[k]) == "markdup" ? &kMarkdupWindowWords : nullptr;
    };
    if (mode == "refusal" && (argc == 7 || argc == 8) && words(7)) {
        const std::string why = window_refusal(num(2), num(3), num(4), num(5), num(6), *words(7));
        printf("%s", why.c_str());
        return why.empty() ? 0 : 3;
    }
    if (mode == "words" && argc == 3 && words(2)) {
        printf("%s\n%s\n", batch_refusal(*words(2)).c_str(), windows_do_not_fit(*words(2), 1000, 10, words(2)->window_needs).c_str());
        return 0;
    }
    return 2;
}
