// file_run.hpp -- one run of a work list in FILE coordinates, and the joining of such runs.  Host only and free of HIP: the engine
// (engine_ctx.hpp), the run planner of the indexed view (view_index_core.hpp) and its CPU test (tests/native/viewidx_host.cpp) read it.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace sbx {

// BGZF blocks [blk0, blk1), inflated-stream offsets [ub, ue).
struct FileRun {
    uint32_t blk0, blk1;
    uint64_t ub, ue;
    bool open_end = false;        // ue is a block boundary in the middle of the record stream (ChainRun::open_end)
    bool operator==(const FileRun& o) const { return blk0 == o.blk0 && blk1 == o.blk1 && ub == o.ub && ue == o.ue && open_end == o.open_end; }
};

// sorted runs joined where they share or touch a block, or lie at most max_gap_blocks whole blocks apart (build_runs joins its chunks
// with a gap of one; what lies between two joined runs is a whole number of records); the end of the joined run is the one that
// reaches furthest, open when that one is
inline std::vector<FileRun> join_runs(std::vector<FileRun> runs, uint32_t max_gap_blocks = 0) {
    std::sort(runs.begin(), runs.end(), [](const FileRun& a, const FileRun& b) { return a.ub != b.ub ? a.ub < b.ub : a.ue < b.ue; });
    std::vector<FileRun> merged;
    for (const FileRun& r : runs) {
        if (!merged.empty() && (uint64_t)r.blk0 <= (uint64_t)merged.back().blk1 + max_gap_blocks) {
            FileRun& m = merged.back();
            if (r.ue > m.ue) { m.ue = r.ue; m.open_end = r.open_end; }
            else if (r.ue == m.ue) m.open_end = m.open_end && r.open_end;
            m.blk1 = std::max(m.blk1, r.blk1);
        } else merged.push_back(r);
    }
    return merged;
}

}  // namespace sbx
