// view_index_core.hpp -- the run planner of the indexed view (sbx_view_run_indexed, engine_view.cpp): from the joined runs the .bai
// names for the regions of a call to the sequence of batches K1 + K2 run over.  Host only and free of HIP; tests/native/viewidx_host.cpp
// drives it with a stream of records written out there.
//
//   runs      build_runs over all regions of the call, the stretch of the region `*` (unmapped_tail), joined (join_runs with a gap
//             of one block, as build_runs joins its chunks).  They ascend in the file and share no block.
//   batch     consecutive WHOLE runs whose blocks inflate to at most the budget: one launch of K1 + K2, U is the concatenation of
//             the runs' blocks and a record's rec_off a work-list offset.
//   piece     a run whose blocks exceed the budget goes alone, cut at block boundaries: every piece but the last is open-ended (the
//             chain stops in front of the record that straddles the cut) and the next piece starts with that record -- exactly
//             as for_each_record_batch continues.  A piece in which not one whole record fits is run again with twice the budget.
//
// The planner cannot know where the chain of an open-ended piece stops; the caller reports it (advance) after every batch.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "file_run.hpp"

namespace sbx {
namespace viewidx {

// the block that holds stream offset u < out_off[n_blocks]
inline uint32_t block_of(const uint64_t* out_off, uint32_t n_blocks, uint64_t u) {
    uint32_t lo = 0, hi = n_blocks;
    while (lo + 1 < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (out_off[mid] <= u) lo = mid; else hi = mid;
    }
    return lo;
}

// The stretch the region `*` adds: from the first record without a reference (stream offset u_unmapped, inside its block) to the
// end of the stream.  Appends nothing when the file holds no such record (u_unmapped at or behind the end).  Blocks behind the
// last byte of the stream (EOF blocks) are not part of the run.
inline void unmapped_tail(const uint64_t* out_off, uint32_t n_blocks, uint64_t u_unmapped, std::vector<FileRun>* runs) {
    const uint64_t total = out_off[n_blocks];
    if (!n_blocks || u_unmapped >= total) return;
    const uint32_t b0 = block_of(out_off, n_blocks, u_unmapped);
    uint32_t b1 = n_blocks;
    while (b1 > b0 + 1 && out_off[b1 - 1] >= total) --b1;
    runs->push_back(FileRun{b0, b1, u_unmapped, total, false});
}

// what the joined runs cost: their blocks and the inflated bytes of those blocks (the device store of the BAM and SAM sinks holds
// at most this much)
inline void runs_cost(const std::vector<FileRun>& runs, const uint64_t* out_off, uint64_t* n_blocks, uint64_t* inflated_bytes) {
    *n_blocks = 0; *inflated_bytes = 0;
    for (const FileRun& r : runs) { *n_blocks += r.blk1 - r.blk0; *inflated_bytes += out_off[r.blk1] - out_off[r.blk0]; }
}

class Planner {
    std::vector<FileRun> runs_;
    const uint64_t* out_off_;
    uint64_t budget_;
    size_t at_ = 0;                 // the first run that is not done
    uint64_t cur_ = 0;              // where its next piece starts
    size_t whole_ = 0;              // the batch handed out last: this many whole runs, or (0) one piece
    bool last_piece_ = false;
    uint64_t block_bytes(const FileRun& r) const { return out_off_[r.blk1] - out_off_[r.blk0]; }

public:
    // runs: joined, ascending; out_off: the block table's inflated offsets ([n_blocks + 1]); budget: inflated bytes per batch (> 0)
    Planner(std::vector<FileRun> runs, const uint64_t* out_off, uint64_t budget)
        : runs_(std::move(runs)), out_off_(out_off), budget_(budget ? budget : 1) {
        if (!runs_.empty()) cur_ = runs_[0].ub;
    }
    uint64_t budget() const { return budget_; }
    // The next batch; false when every run is done.
    bool next(std::vector<FileRun>* batch) {
        batch->clear();
        if (at_ >= runs_.size()) return false;
        const FileRun& r = runs_[at_];
        if (cur_ == r.ub && block_bytes(r) <= budget_) {
            uint64_t sum = 0;
            size_t k = at_;
            while (k < runs_.size() && sum + block_bytes(runs_[k]) <= budget_) { sum += block_bytes(runs_[k]); batch->push_back(runs_[k]); ++k; }
            whole_ = k - at_;
            return true;
        }
        whole_ = 0;
        const uint32_t b0 = block_of(out_off_ + r.blk0, r.blk1 - r.blk0, cur_) + r.blk0;
        uint32_t b1 = b0 + 1;
        while (b1 < r.blk1 && out_off_[b1] < out_off_[b0] + budget_) ++b1;       // (the first boundary at or behind the budget)
        last_piece_ = b1 >= r.blk1 || out_off_[b1] >= r.ue;
        batch->push_back(last_piece_ ? FileRun{b0, r.blk1, cur_, r.ue, r.open_end} : FileRun{b0, b1, cur_, out_off_[b1], true});
        return true;
    }
    // After the batch of next() ran: `stop` is the stream offset behind its last described record (RecordBatch::next; of no
    // meaning for whole runs).  Returns false when the batch held not one whole record and is to be run again, longer: the
    // caller then discards it.
    bool advance(uint64_t stop) {
        if (whole_) {
            at_ += whole_;
        } else if (last_piece_) {
            ++at_;
        } else {
            if (stop <= cur_) { budget_ *= 2; return false; }
            cur_ = stop;
            return true;
        }
        if (at_ < runs_.size()) cur_ = runs_[at_].ub;
        return true;
    }
};

}  // namespace viewidx
}  // namespace sbx
