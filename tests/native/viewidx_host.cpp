// viewidx_host.cpp -- view_index_core.hpp and file_run.hpp compiled for the host (tests/test_view_index_core_cpu.py), plainly and
// under ASan + UBSan.  All input comes from stdin as whitespace-separated numbers.
//   viewidx_host plan   n_blocks out_off[0..n]  budget  n_runs {blk0 blk1 ub ue}*  n_records rec_off[0..n_records]
//                       The planner driven the way read_batches drives it; the chain walk of K2 is played by the record list:
//                       an open-ended piece stops at the first record at or behind its start that ends behind its end.
//                       Prints per batch "B|D  {blk0 blk1 ub ue open}+  stop" (D: discarded, run again longer), then "budget N".
//   viewidx_host join   gap n_runs {blk0 blk1 ub ue open}*      prints the joined runs, one per line
//   viewidx_host tail   n_blocks out_off[0..n] u_unmapped       prints the run of `*`, or "none"
//   viewidx_host cost   n_blocks out_off[0..n] n_runs {blk0 blk1 ub ue}*     prints blocks and inflated bytes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../sambamba_amd/csrc/view_index_core.hpp"

using namespace sbx;

static bool rd(unsigned long long* v) { return scanf("%llu", v) == 1; }
static unsigned long long need() {
    unsigned long long v = 0;
    if (!rd(&v)) { fprintf(stderr, "viewidx_host: input ends early\n"); exit(2); }
    return v;
}
static std::vector<uint64_t> read_table() {
    const size_t n = (size_t)need();
    std::vector<uint64_t> t(n + 1);
    for (auto& x : t) x = need();
    return t;
}
static std::vector<FileRun> read_runs(bool with_open) {
    const size_t n = (size_t)need();
    std::vector<FileRun> runs;
    for (size_t k = 0; k < n; ++k) {
        FileRun r{};
        r.blk0 = (uint32_t)need(); r.blk1 = (uint32_t)need(); r.ub = need(); r.ue = need();
        r.open_end = with_open ? need() != 0 : false;
        runs.push_back(r);
    }
    return runs;
}
static void print_run(const FileRun& r) { printf("%u %u %llu %llu %d", r.blk0, r.blk1, (unsigned long long)r.ub, (unsigned long long)r.ue, r.open_end ? 1 : 0); }

int main(int argc, char** argv) {
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "plan")) {
        const std::vector<uint64_t> off = read_table();
        const uint64_t budget = need();
        const std::vector<FileRun> runs = read_runs(false);
        const size_t n_rec = (size_t)need();
        std::vector<uint64_t> rec(n_rec + 1);
        for (auto& x : rec) x = need();
        viewidx::Planner planner(runs, off.data(), budget);
        std::vector<FileRun> batch;
        int guard = 0;
        while (planner.next(&batch)) {
            if (++guard > 10000) { fprintf(stderr, "viewidx_host: the plan does not end\n"); return 3; }
            uint64_t stop = batch.back().ue;
            if (batch.size() == 1 && batch[0].open_end)
                for (size_t k = 0; k < n_rec; ++k)
                    if (rec[k] >= batch[0].ub && rec[k + 1] > batch[0].ue) { stop = rec[k]; break; }
            const bool kept = planner.advance(stop);
            printf(kept ? "B" : "D");
            for (const FileRun& r : batch) { printf("  "); print_run(r); }
            printf("  %llu\n", (unsigned long long)stop);
        }
        printf("budget %llu\n", (unsigned long long)planner.budget());
        return 0;
    }
    if (!strcmp(cmd, "join")) {
        const uint32_t gap = (uint32_t)need();
        for (const FileRun& r : join_runs(read_runs(true), gap)) { print_run(r); printf("\n"); }
        return 0;
    }
    if (!strcmp(cmd, "tail")) {
        const std::vector<uint64_t> off = read_table();
        std::vector<FileRun> runs;
        viewidx::unmapped_tail(off.data(), (uint32_t)off.size() - 1, need(), &runs);
        if (runs.empty()) printf("none\n");
        else { print_run(runs[0]); printf("\n"); }
        return 0;
    }
    if (!strcmp(cmd, "cost")) {
        const std::vector<uint64_t> off = read_table();
        uint64_t nb = 0, bytes = 0;
        viewidx::runs_cost(read_runs(false), off.data(), &nb, &bytes);
        printf("%llu %llu\n", (unsigned long long)nb, (unsigned long long)bytes);
        return 0;
    }
    fprintf(stderr, "usage: viewidx_host plan|join|tail|cost\n");
    return 2;
}
