// valid.hpp -- launcher of K19 (valid.hip): the validity of the records of a batch (valid_core.hpp).
#pragma once
#include "kernels.hpp"
#include "valid_core.hpp"

namespace sbx {

// words K19 adds to over the batches of a file: records of class k, k < validc::kClasses, then the invalid records; behind them
// the lowest ordinal (rec_base + index in the batch) of an invalid record so far, kValidNone when there is none
enum ValidAcc : uint32_t { kValidAccInvalid = validc::kClasses, kValidAccFirst = validc::kClasses + 1, kValidAccWords = validc::kClasses + 2 };
constexpr unsigned long long kValidNone = ~0ull;

struct ValidArgs {
    const uint8_t* U;               // inflated bytes of the batch
    const RecDesc* desc;            // its records (only rec_off is read)
    uint64_t n;                     // records of the batch
    uint64_t u_end;                 // no byte at or behind this offset of U is read
    uint64_t rec_base;              // ordinal of the batch's first record in the file
    uint16_t* mask;                 // [n] out: validc::record_mask of every record; may be null
    unsigned long long* acc;        // [kValidAccWords]
};
// K19
void launch_valid_masks(const ValidArgs& a, hipStream_t stream);

}  // namespace sbx
