// stream_patch_host.cpp -- the patch offset of K21's plan (streamc::plan_record, sambamba_amd/csrc/stream_core.hpp) on the CPU, next to
// stream_host.cpp which checks the bin patch at its default offset: with the flag patch at byte 18 (streamc::kFlagOffset) a record is
// put through two adjoining windows whose common edge lies at dest + 17, + 18, + 19 and + 20 -- in front of the pair, between its
// two bytes, behind it -- and through windows cut at both ends, against a byte-wise restatement with guard bytes around the window:
// no byte outside the window is written, none twice, every byte that belongs exactly once with the right value, wrote() is their
// number, and over the two windows the record arrives whole with exactly bytes 18 and 19 replaced.  The defaulted parameter must
// plan what an explicit 14 plans.
//   stream_patch_host       prints "cases N split M" (M: windows that received exactly one of the two patched bytes)
// Exit 0: all as stated; 1: a difference (said on stderr).
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sambamba_amd/csrc/stream_core.hpp"

using namespace sbx;

namespace {

constexpr size_t kGuard = 32;
constexpr uint8_t kGuardByte = 0xA5, kUnset = 0x5A;

uint8_t rec_byte(uint64_t id, uint64_t j) { return (uint8_t)((id * 131 + j * 7 + 3) % 127); }

// one record against one window; adds the bytes the window received to `whole` (the record as it arrives over all its windows)
bool one_window(uint64_t dest, uint64_t len, uint64_t w0, uint64_t w1, uint32_t val, uint32_t off, uint64_t id, std::vector<int>* whole,
                bool* split) {
    const size_t W = (size_t)(w1 - w0);
    std::vector<uint8_t> got(W + 2 * kGuard, kGuardByte), want(W + 2 * kGuard, kGuardByte);
    std::vector<uint32_t> writes(got.size(), 0);
    for (size_t k = 0; k < W; ++k) got[kGuard + k] = want[kGuard + k] = kUnset;
    uint64_t belong = 0;
    uint32_t patched_in = 0;
    for (uint64_t j = 0; j < len; ++j) {
        const uint64_t at = dest + j;
        if (at < w0 || at >= w1) continue;
        uint8_t v = rec_byte(id, j);
        if (val != streamc::kNoPatch && (j == off || j == off + 1)) { v = (uint8_t)(val >> (8 * (j - off))); ++patched_in; }
        want[kGuard + (size_t)(at - w0)] = v;
        ++belong;
    }
    *split = patched_in == 1;
    streamc::PackPlan p;
    streamc::plan_record(dest, len, w0, w1, val, &p, off);
    for (uint32_t k = 0; k < p.n_spans; ++k) {
        if (!p.span[k].len || p.span[k].dst + p.span[k].len > W || p.span[k].src + p.span[k].len > len) { fprintf(stderr, "span outside\n"); return false; }
        for (uint64_t b = 0; b < p.span[k].len; ++b) {
            const size_t at = kGuard + (size_t)(p.span[k].dst + b);
            got[at] = rec_byte(id, p.span[k].src + b);
            ++writes[at];
        }
    }
    for (uint32_t k = 0; k < p.n_bytes; ++k) {
        if (p.byte_dst[k] >= W) { fprintf(stderr, "patch byte outside\n"); return false; }
        got[kGuard + (size_t)p.byte_dst[k]] = p.byte_val[k];
        ++writes[kGuard + (size_t)p.byte_dst[k]];
    }
    bool ok = got == want && p.wrote() == belong;
    uint64_t written = 0;
    for (size_t k = 0; k < writes.size(); ++k) {
        const bool inside = k >= kGuard && k < kGuard + W;
        if (writes[k] > 1 || (!inside && writes[k])) ok = false;
        written += writes[k];
    }
    if (written != belong) ok = false;
    if (!ok) {
        fprintf(stderr, "difference: dest=%llu len=%llu w=[%llu,%llu) val=%x off=%u wrote=%llu belong=%llu\n", (unsigned long long)dest,
                (unsigned long long)len, (unsigned long long)w0, (unsigned long long)w1, val, off, (unsigned long long)p.wrote(),
                (unsigned long long)belong);
        return false;
    }
    for (uint64_t j = 0; j < len; ++j) {
        const uint64_t at = dest + j;
        if (at >= w0 && at < w1) (*whole)[(size_t)j] = got[kGuard + (size_t)(at - w0)];
    }
    return true;
}

bool same_plan(const streamc::PackPlan& a, const streamc::PackPlan& b) {
    if (a.n_spans != b.n_spans || a.n_bytes != b.n_bytes) return false;
    for (uint32_t k = 0; k < a.n_spans; ++k)
        if (a.span[k].dst != b.span[k].dst || a.span[k].src != b.span[k].src || a.span[k].len != b.span[k].len) return false;
    for (uint32_t k = 0; k < a.n_bytes; ++k)
        if (a.byte_dst[k] != b.byte_dst[k] || a.byte_val[k] != b.byte_val[k]) return false;
    return true;
}

}  // namespace

int main() {
    const uint32_t off = streamc::kFlagOffset;
    if (off != 18 || streamc::kBinOffset != 14) { fprintf(stderr, "offsets\n"); return 1; }
    uint64_t cases = 0, n_split = 0, id = 0;
    for (uint64_t len : {36ull, 37ull, 52ull, 300ull})
        for (uint64_t dest : {0ull, 5ull, 65280ull - 18, 1000003ull})
            for (uint32_t val : {streamc::kNoPatch, 0x0200u, 0x0663u, 0xFFFFu, 0u})
                for (uint64_t d = 17; d <= 20; ++d) {
                    const uint64_t edge = dest + d;
                    // the two windows that meet at the edge: one reaching back in front of the record, one cut inside it, and the
                    // windows behind the edge likewise
                    for (uint64_t back : {edge, (uint64_t)7}) {
                        for (uint64_t ahead : {len + 50, (uint64_t)9}) {
                            std::vector<int> whole((size_t)len, -1);
                            const uint64_t w0 = edge - (back < edge ? back : edge);
                            bool s1 = false, s2 = false;
                            if (!one_window(dest, len, w0, edge, val, off, id, &whole, &s1)) return 1;
                            if (!one_window(dest, len, edge, edge + ahead, val, off, id, &whole, &s2)) return 1;
                            cases += 2;
                            n_split += (s1 ? 1 : 0) + (s2 ? 1 : 0);
                            if ((s1 != s2) || (val != streamc::kNoPatch && s1 != (d == 19))) { fprintf(stderr, "split at d=%llu\n", (unsigned long long)d); return 1; }
                            // what arrived over the two windows: the record with exactly the pair replaced
                            for (uint64_t j = 0; j < len; ++j) {
                                const uint64_t at = dest + j;
                                if (at < w0 || at >= edge + ahead) continue;
                                int v = rec_byte(id, j);
                                if (val != streamc::kNoPatch && (j == off || j == off + 1)) v = (uint8_t)(val >> (8 * (j - off)));
                                if (whole[(size_t)j] != v) { fprintf(stderr, "byte %llu of the record arrived as %d\n", (unsigned long long)j, whole[(size_t)j]); return 1; }
                            }
                            ++id;
                        }
                    }
                    // the defaulted parameter is the bin offset
                    streamc::PackPlan a, b;
                    streamc::plan_record(dest, len, edge - 3, edge + 40, val, &a);
                    streamc::plan_record(dest, len, edge - 3, edge + 40, val, &b, streamc::kBinOffset);
                    if (!same_plan(a, b)) { fprintf(stderr, "the default offset is not 14\n"); return 1; }
                }
    printf("cases %llu split %llu\n", (unsigned long long)cases, (unsigned long long)n_split);
    return 0;
}
