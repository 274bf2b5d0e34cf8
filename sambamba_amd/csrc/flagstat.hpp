// flagstat.hpp -- launcher of K8 (flagstat.hip), `sambamba flagstat` on the described records of a batch.
#pragma once
#include "kernels.hpp"

namespace sbx {

// adds the 26 counters of sbx_flagstat_counts over records [0, n_records) of a batch to d_counts
void launch_flagstat(const uint8_t* d_U, const RecDesc* d_desc, const int32_t* d_rec_ref, uint64_t n_records, unsigned long long* d_counts,
                     hipStream_t stream);

}  // namespace sbx
