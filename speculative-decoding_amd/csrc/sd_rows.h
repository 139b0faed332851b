// sd_rows.h — the row table of specdec_kernels.hip for the library's other units (sample_distinct.hip):
// the (max, Σexp) pair and, under a top-k / nucleus processor, the keep predicate of each of `rows`
// processed rows, formed as the tree verifies form theirs (the launch-per-phase threshold search, k_stats,
// k_tree_rowstat; sd_row_table.inc).  A probability read through this table is the value the verifies read.
// Hidden visibility: not part of the C ABI.  A unit that calls these links with specdec_kernels.
#pragma once
#include "sd_device.h"
#include "sd_host.h"

namespace sd_host __attribute__((visibility("hidden"))) {

struct RowTable {
    const float2* stat;          // [rows]
    const sd::RowKeep* keep;     // [rows], written under a top-k / nucleus processor only
};

// specdec_kernels.hip's valid_proc: the processor checks every entry point shares
bool row_table_valid_proc(const sd_processor& proc);
// bytes at the front of a workspace that row_table uses: the common counter block, then its own arrays
size_t row_table_size(int32_t rows, int32_t vocab);
// launches on `stream`; row r at logits + r * stride_r elements; the caller has checked dtype and processor
int32_t row_table(const void* logits, int64_t stride_r, int32_t rows, int32_t vocab, int32_t dtype, const sd_processor& proc,
                  int32_t* status_or, void* workspace, RowTable* out, void* stream);

}  // namespace sd_host
