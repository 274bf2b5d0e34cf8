// cli_common.hpp -- what every part of sbx-depth shares: the parsed options, the buffered output, the error type, the clock, the
// walk over the active ranges of the resident run, how a context is set up like the first one, the hand-over between stage /
// device threads (StageSync, StageThreads) and the cutter of position slices.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <ctime>
#include <mutex>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/sbx_depth.h"

namespace sbx {

struct Options {
    std::string mode, filter, output_fn, regions;
    std::vector<std::string> bams;
    bool has_filter = false, has_regions = false, report_zero = false;
    bool annotate = false, combined = false, fix_mate = false;
    int n_threads = 0, min_bq = 0;
    double min_cov = 0.0, max_cov = 1e50;
    std::vector<uint32_t> thresholds;
    unsigned long long window = 0, overlap = 0;
    int gpus = 0;             // --gpus N: shard the job by position over N devices (an extension; SBX_DEVICES lists the ordinals)
};

constexpr size_t kMaxCliThresholds = 64;

struct Out {
    FILE* fp = stdout;
    std::string buf;
    void put(const char* s, size_t n) { buf.append(s, n); if (buf.size() > (4u << 20)) flush(); }
    void put(const std::string& s) { put(s.data(), s.size()); }
    void flush() { if (!buf.empty()) fwrite(buf.data(), 1, buf.size(), fp); buf.clear(); }
};

inline char* u64toa(uint64_t v, char* end) {  // writes backwards, returns start
    do { *--end = (char)('0' + v % 10); v /= 10; } while (v);
    return end;
}

struct Fail { std::string msg; };
inline void check(sbx_ctx* c, int rc) { if (rc != SBX_OK) throw Fail{sbx_last_error(c)}; }
inline double now() { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return t.tv_sec + 1e-9 * t.tv_nsec; }
inline uint64_t ref_len(sbx_ctx* c, int r) { return (uint64_t)std::max<int64_t>(0, sbx_ref_length(c, r)); }
inline uint64_t total_positions(sbx_ctx* c, int n_ref) { uint64_t t = 0; for (int r = 0; r < n_ref; ++r) t += ref_len(c, r); return t; }

// fn(b, e) for every active range (tiles with admitted reads) of contig r of the resident run, clipped to [from, end), in order.
// A fn that returns bool ends the walk by returning false.
constexpr uint64_t kNoEnd = ~0ULL;
template <class F> void for_each_active_range(sbx_ctx* c, uint32_t r, uint64_t from, uint64_t end, F&& fn) {
    for (;;) {
        uint64_t b, e;
        check(c, sbx_next_active_range(c, r, from, &b, &e));
        if (b == ~0ULL || b >= end) return;
        b = std::max(b, from);
        e = std::min(e, end);
        if constexpr (std::is_void_v<decltype(fn(b, e))>) fn(b, e);
        else if (!fn(b, e)) return;
        from = e;
    }
}
inline bool has_active_range(sbx_ctx* c, uint32_t r) {       // ... does contig r have one at all (a single probe)
    uint64_t b = 0, e = 0;
    check(c, sbx_next_active_range(c, r, 0, &b, &e));
    return b != ~0ULL;
}

// filter, parameters and (when given) the merged -L regions of the job: the same for every context that works on it
inline void configure_context(sbx_ctx* c, const sbx_filter& filt, int mode_id, const Options& o, const std::vector<sbx_region>* merged) {
    check(c, sbx_set_filter(c, &filt));
    check(c, sbx_set_params(c, mode_id, (uint8_t)o.min_bq, o.fix_mate, o.combined, (uint32_t)o.window, (uint32_t)o.overlap,
                            o.thresholds.data(), (int)o.thresholds.size()));
    if (merged && !merged->empty()) check(c, sbx_set_regions(c, merged->data(), merged->size()));
}
// another context on the same files, set up like the first one
inline sbx_ctx* open_configured(const std::vector<const char*>& paths, int device, const sbx_filter& filt, int mode_id, const Options& o,
                                const std::vector<sbx_region>* merged) {
    char e[512] = {0};
    sbx_ctx* c = sbx_open(paths.data(), (int)paths.size(), device, e, sizeof e);
    if (!c) throw Fail{e};
    try { configure_context(c, filt, mode_id, o, merged); }
    catch (...) { sbx_close(c); throw; }
    return c;
}

// What threads that hand work to each other share: one mutex, one condition variable and the FIRST failure.  Every wait ends
// when some thread has failed, so a failure anywhere releases everybody.
struct StageSync {
    std::mutex mu;
    std::condition_variable cv;
    std::string failure;
    int failure_code = SBX_OK;
    const char* anonymous;               // the message of a failure that has none
    explicit StageSync(const char* anonymous_failure) : anonymous(anonymous_failure) {}
    void fail(const std::string& m, int code = SBX_EINVAL) {
        std::lock_guard<std::mutex> g(mu);
        if (failure.empty()) { failure = m.empty() ? std::string(anonymous) : m; failure_code = code; }
        cv.notify_all();
    }
    template <class P> bool wait_for(P&& pred) {       // false: somebody failed
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return !failure.empty() || pred(); });
        return failure.empty();
    }
    // publish: set() runs under the mutex, then everybody who waits looks again
    template <class F> void mark(F&& set) { std::lock_guard<std::mutex> g(mu); set(); cv.notify_all(); }
};

// The threads of a StageSync.  Whatever leaves the scope -- an exception of any kind included -- first releases them (unless the
// owner said that all of them are past their last wait: `regular`), then joins them.  Threads start inside the scope of the guard that
// joins them: an exception while the second or third one is being created -- thread exhaustion -- must not destroy a running std::thread.
struct StageThreads {
    StageSync& sync;
    std::vector<std::thread> th;
    bool regular = false;
    explicit StageThreads(StageSync& s) : sync(s) {}
    template <class F> void start(F&& f) { th.emplace_back(std::forward<F>(f)); }
    void join() { for (auto& t : th) if (t.joinable()) t.join(); }
    ~StageThreads() { if (!regular) sync.fail("aborted"); join(); }
};

// A stretch of a contig that one run computes (sbx_run_interval) and prints.  print_end: the last slice of a contig prints to
// 0xFFFFFFFF -- the columns of alignments hanging over the contig end.
struct Slice { uint32_t ref; uint64_t beg, end, print_end; size_t owner; };
constexpr uint64_t kPrintToEnd = 0xFFFFFFFFull;
// Every share [beg, end) of a contig in equal slices of about `want` positions (SBX_SLICE_POSITIONS overrides), cut at multiples of 1024
inline std::vector<Slice> cut_slices(sbx_ctx* c, const std::vector<Slice>& shares, uint64_t want) {
    if (const char* e = getenv("SBX_SLICE_POSITIONS")) want = std::max<uint64_t>(1024, strtoull(e, nullptr, 10));
    want = (want + 1023) / 1024 * 1024;
    std::vector<Slice> sl;
    for (const Slice& sh : shares) {
        if (sh.end <= sh.beg) continue;
        const uint64_t len = ref_len(c, (int)sh.ref), span = sh.end - sh.beg;
        const uint64_t n = (span + want - 1) / want, step = ((span + n - 1) / n + 1023) / 1024 * 1024;
        for (uint64_t b = sh.beg; b < sh.end; b += step) {
            const uint64_t e = std::min(sh.end, b + step);
            sl.push_back({sh.ref, b, e, e == len ? kPrintToEnd : e, sh.owner});
        }
    }
    return sl;
}

}  // namespace sbx
