// mergewin_host.cpp -- the pieces of a rewritten record clipped to a window (sambamba_amd/csrc/mergewin_core.hpp) on the CPU
// (tests/test_merge_window_core_cpu.py), through the very functions K11c (merge.hip) compiles.  Built with -fsanitize=address,undefined.
//   mergewin_host exhaustive LO HI   records of old length LO .. HI (the test: 36 .. 80, in three calls) with 0, 1 and 2 patches,
//                                 old and new id lengths 0 .. 5 each, the patches directly behind byte 36, in the middle, adjacent
//                                 to each other and at the record's end;
//                                 every dest in 0 .. 6 and, for spans of 1, 2 and 3 pieces of 7 bytes, every window [k span,
//                                 (k + 1) span) that lies in front of, on or behind the record (the windows of plan_windows; the
//                                 span of one piece puts an edge at every byte of the record, the longer spans not at every
//                                 alignment).  The plan of every (record, dest, window) is executed into a guard-padded
//                                 window and must reproduce the slice of the reference rewrite -- K11b's byte order, restated
//                                 below without the core -- writing each byte once and none outside the window.  stdout: one line
//                                 "records R plans P stretches S max M"; exit status 1 and a line on stderr for the first failure.
//   mergewin_host one OLD_LEN DEST W0 W1 [AT OLD NEW [AT OLD NEW]]   -> the plan, one line "kind src dst len" per stretch
//   mergewin_host words           the three refusals of the windowed writer in merge's words, one per line: batch_refusal,
//                                 window_refusal for bytes [65280, 130560) with a 100-byte header, 65279 bytes and 2 mismatches, and
//                                 windows_do_not_fit for 1000 bytes needed, 10 free and the command's own window_needs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sambamba_amd/csrc/mergewin_core.hpp"

using namespace sbx;
using namespace sbx::mergewin;

namespace {

constexpr uint64_t kPiece = 7, kGuard = 8, kMaxSpan = 3 * kPiece;
constexpr uint32_t kNewRef = 0x0A0B0C0D, kNewNext = 0x51525354;

uint32_t ld32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

struct Record {
    std::vector<uint8_t> old_bytes, blob, want;       // the record as read, the rename blob, the reference rewrite
    Patch patch[kMaxPatches];
    uint32_t np = 0;
    uint32_t old_len() const { return (uint32_t)old_bytes.size(); }
    uint32_t new_len() const { return (uint32_t)want.size(); }
};

// the record as read, and what K11b writes for it: the 36 fixed bytes with the three words replaced, then source, new id, source,
// new id, tail -- byte by byte, without clip_to_piece and without for_each_stretch
Record make_record(uint32_t old_len, uint32_t np, const uint32_t* at, const uint32_t* ol, const uint32_t* nl) {
    Record r;
    r.old_bytes.resize(old_len);
    for (uint32_t j = 0; j < old_len; ++j) r.old_bytes[j] = (uint8_t)(0x20 + (j * 5 + old_len) % 0x5B);
    const uint32_t bs = old_len - 4;
    for (int b = 0; b < 4; ++b) r.old_bytes[b] = (uint8_t)(bs >> (8 * b));
    r.np = np;
    uint32_t new_len = old_len;
    r.blob.assign(3, 0xB0);                                        // (a new id does not start at offset 0 of the blob)
    for (uint32_t k = 0; k < np; ++k) {
        r.patch[k] = Patch{at[k], ol[k], nl[k], (uint32_t)r.blob.size()};
        for (uint32_t b = 0; b < nl[k]; ++b) r.blob.push_back((uint8_t)(0xC0 + 16 * k + b));
        r.blob.push_back(0xBF);
        new_len += nl[k];
        new_len -= ol[k];
    }
    std::vector<uint8_t>& w = r.want;
    for (uint32_t b = 0; b < 36; ++b) {
        const uint32_t word = b / 4;
        const uint32_t v = word == 0 ? new_len - 4 : word == 1 ? kNewRef : word == 6 ? kNewNext : ld32(&r.old_bytes[4 * word]);
        w.push_back((uint8_t)(v >> (8 * (b % 4))));
    }
    uint32_t s = 36;
    for (uint32_t k = 0; k < np; ++k) {
        for (; s < at[k]; ++s) w.push_back(r.old_bytes[s]);
        for (uint32_t b = 0; b < nl[k]; ++b) w.push_back(r.blob[r.patch[k].new_off + b]);
        s = at[k] + ol[k];
    }
    for (; s < old_len; ++s) w.push_back(r.old_bytes[s]);
    if (w.size() != new_len) { fprintf(stderr, "the restatement is inconsistent\n"); exit(2); }
    return r;
}

struct Totals { unsigned long long records = 0, plans = 0, stretches = 0, most = 0; };

// every dest and every window for one record; false: a line on stderr says what failed
bool check_record(const Record& r, Totals* t) {
    static uint8_t win[kMaxSpan + 2 * kGuard], cnt[kMaxSpan + 2 * kGuard];     // the guard-padded window; how often a byte was written
    static bool fresh = true;
    if (fresh) { memset(win, 0xEE, sizeof win); memset(cnt, 0, sizeof cnt); fresh = false; }       // (every plan leaves them so)
    ++t->records;
    const uint32_t old_len = r.old_len(), new_len = r.new_len();
    for (uint64_t dest = 0; dest < kPiece; ++dest)
        for (uint64_t pieces = 1; pieces <= 3; ++pieces) {
            const uint64_t span = pieces * kPiece;
            for (uint64_t w0 = 0; w0 < dest + new_len + span; w0 += span) {
                const uint64_t w1 = w0 + span;
                Stretch st[kMaxStretches + 1];
                const uint32_t n = plan_record_window(old_len, new_len, r.patch, r.np, dest, w0, w1, st);
                ++t->plans;
                t->stretches += n;
                if (n > t->most) t->most = n;
                auto fail = [&](const char* what, uint64_t a, uint64_t b) {
                    fprintf(stderr, "%s (%llu, %llu): old_len %u new_len %u patches %u dest %llu window [%llu, %llu)", what, (unsigned long long)a,
                            (unsigned long long)b, old_len, new_len, r.np, (unsigned long long)dest, (unsigned long long)w0, (unsigned long long)w1);
                    for (uint32_t k = 0; k < r.np; ++k) fprintf(stderr, " patch(at %u old %u new %u)", r.patch[k].at, r.patch[k].old_len, r.patch[k].new_len);
                    fprintf(stderr, "\n");
                    return false;
                };
                if (n > kMaxStretches) return fail("too many stretches", n, kMaxStretches);
                // what the window holds of the record
                sortc::PieceClip whole;
                const uint64_t belongs = sortc::clip_to_piece(dest, dest + new_len, w0, w1, &whole) ? whole.len : 0;
                uint64_t written = 0;
                for (uint32_t q = 0; q < n; ++q) {
                    const Stretch& x = st[q];
                    if (!x.len) return fail("an empty stretch", q, 0);
                    if (x.dst + x.len > span) return fail("a stretch leaves the window", x.dst, x.len);
                    const uint64_t limit = x.kind == kStretchFixed ? kFixedBytes : x.kind == kStretchSource ? old_len : r.blob.size();
                    if (x.kind > kStretchBlob || x.src + x.len > limit) return fail("a stretch leaves its source", x.src, x.len);
                    if (x.kind == kStretchSource && x.src < kFixedBytes) return fail("a source stretch reads the fixed part", x.src, x.len);
                    for (uint64_t b = 0; b < x.len; ++b) {
                        uint8_t v;
                        if (x.kind == kStretchFixed) {
                            const uint32_t fb = (uint32_t)(x.src + b);
                            v = fixed_byte(fb, new_len - 4, kNewRef, kNewNext, ld32(&r.old_bytes[4 * (fb >> 2)]));
                        } else {
                            v = x.kind == kStretchSource ? r.old_bytes[x.src + b] : r.blob[x.src + b];
                        }
                        const uint64_t g = kGuard + x.dst + b, p = w0 + x.dst + b;       // in the padded window; in the stream
                        if (p < dest || p >= dest + new_len) return fail("a byte written that is not the record's", g, p);
                        if (cnt[g]) return fail("a byte of the window written twice", g, p);
                        if (v != r.want[p - dest]) return fail("a wrong byte", g, v);
                        win[g] = v;
                        cnt[g] = 1;
                        ++written;
                    }
                }
                // every byte written lay inside the window and inside the record, none twice: with the count, each exactly once
                if (written != belongs) return fail("bytes of the window left out", written, belongs);
                for (uint32_t q = 0; q < n; ++q)
                    for (uint64_t b = 0; b < st[q].len; ++b) { win[kGuard + st[q].dst + b] = 0xEE; cnt[kGuard + st[q].dst + b] = 0; }
            }
        }
    // every plan has cleared what it wrote: the window and its guards are as they were
    for (uint64_t g = 0; g < sizeof win; ++g)
        if (win[g] != 0xEE || cnt[g]) { fprintf(stderr, "byte %llu of the padded window was left written\n", (unsigned long long)g); return false; }
    return true;
}

int exhaustive(uint32_t lo, uint32_t hi) {
    Totals t;
    for (uint32_t old_len = lo; old_len <= hi; ++old_len) {
        if (!check_record(make_record(old_len, 0, nullptr, nullptr, nullptr), &t)) return 1;
        // one patch: directly behind byte 36, in the middle, at the record's end
        for (uint32_t o = 0; o <= 5; ++o)
            for (uint32_t nl = 0; nl <= 5; ++nl) {
                if (36 + o > old_len) continue;
                const uint32_t end = old_len - o, mid = (36 + end) / 2;
                uint32_t seen[3], ns = 0;
                for (uint32_t at : {36u, mid, end}) {
                    bool dup = false;
                    for (uint32_t q = 0; q < ns; ++q) dup = dup || seen[q] == at;
                    if (dup) continue;
                    seen[ns++] = at;
                    if (!check_record(make_record(old_len, 1, &at, &o, &nl), &t)) return 1;
                }
            }
        // two patches: both behind byte 36 and adjacent; one behind byte 36 and one at the end; adjacent at the end; apart in the middle
        for (uint32_t o1 = 0; o1 <= 5; ++o1)
            for (uint32_t n1 = 0; n1 <= 5; ++n1)
                for (uint32_t o2 = 0; o2 <= 5; ++o2)
                    for (uint32_t n2 = 0; n2 <= 5; ++n2) {
                        if (36 + o1 + o2 > old_len) continue;
                        const uint32_t ol[2] = {o1, o2}, nl[2] = {n1, n2};
                        const uint32_t end2 = old_len - o2;
                        const uint32_t layouts[4][2] = {{36, 36 + o1}, {36, end2}, {end2 - o1, end2}, {36 + (end2 - o1 - 36) / 3, end2 - (end2 - o1 - 36) / 3}};
                        for (uint32_t k = 0; k < 4; ++k) {
                            bool dup = false;
                            for (uint32_t q = 0; q < k; ++q) dup = dup || (layouts[q][0] == layouts[k][0] && layouts[q][1] == layouts[k][1]);
                            if (dup) continue;
                            if (layouts[k][0] < 36 || layouts[k][0] + o1 > layouts[k][1] || layouts[k][1] + o2 > old_len) { fprintf(stderr, "a layout is off\n"); return 2; }
                            if (!check_record(make_record(old_len, 2, layouts[k], ol, nl), &t)) return 1;
                        }
                    }
    }
    printf("records %llu plans %llu stretches %llu max %llu\n", t.records, t.plans, t.stretches, t.most);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    auto num = [&](int k) { return strtoull(argv[k], nullptr, 10); };
    if (mode == "exhaustive" && argc == 4 && num(2) >= 36 && num(3) <= 4096) return exhaustive((uint32_t)num(2), (uint32_t)num(3));
    if (mode == "one" && (argc == 6 || argc == 9 || argc == 12)) {
        Patch p[kMaxPatches];
        const uint32_t np = (uint32_t)(argc - 6) / 3;
        uint32_t new_len = (uint32_t)num(2);
        for (uint32_t k = 0; k < np; ++k) {
            p[k] = Patch{(uint32_t)num(6 + 3 * k), (uint32_t)num(7 + 3 * k), (uint32_t)num(8 + 3 * k), 1000 * (k + 1)};
            new_len += p[k].new_len - p[k].old_len;
        }
        Stretch st[kMaxStretches];
        const uint32_t n = plan_record_window((uint32_t)num(2), new_len, p, np, num(3), num(4), num(5), st);
        for (uint32_t q = 0; q < n; ++q)
            printf("%u %llu %llu %llu\n", st[q].kind, (unsigned long long)st[q].src, (unsigned long long)st[q].dst, (unsigned long long)st[q].len);
        return 0;
    }
    if (mode == "words" && argc == 2) {
        const sortc::WindowWords& w = sortc::kMergeWindowWords;
        printf("%s\n%s\n%s\n", sortc::batch_refusal(w).c_str(), sortc::window_refusal(65280, 130560, 100, 65279, 2, w).c_str(),
               sortc::windows_do_not_fit(w, 1000, 10, w.window_needs).c_str());
        return 0;
    }
    return 2;
}
