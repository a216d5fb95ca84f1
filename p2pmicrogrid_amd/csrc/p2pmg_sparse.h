// p2pmg_sparse.h — the host side of the sparse table checkpoints (p2pmg_get_q_sparse, p2pmg_set_q_sparse)
// that needs no device: the check of an uploaded sparse form and the walk of a table range in staging
// runs.  Pure functions with no HIP call, so a program without a GPU can check them under a sanitizer
// (tests/sparse_check.cpp, built and run by tests/test_cpu_sparse_tables.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "p2pmg.h"

namespace p2pmg {

// bytes one stored row takes in staging and on the host: its int32 index and its n_actions values
inline size_t sparse_row_bytes(int n_actions, int host_dtype) {
  return sizeof(int32_t) + (size_t)n_actions * (host_dtype == P2PMG_Q_F64 ? 8 : 4);
}

// Check the sparse form of `count` tables before any of it is uploaded: every n_rows[k] in [0, n_states],
// every index in [0, n_states), indices strictly ascending inside each table (so no duplicates: the
// scatter has no write race).  Reads n_rows[0 .. count) and rows[0 .. sum of n_rows) and nothing else; a
// bad n_rows[k] ends the check before any index of table k or later is read.  rows may be null when
// every table is empty.  Returns null and the total in *total, or what is wrong (*total is then unset).
const char* sparse_validate(const int64_t* n_rows, const int32_t* rows, int count, size_t n_states, int64_t* total);

// Tables [first, first + count) of the range, relative to its start, whose `rows` stored rows begin at
// row0 of the range's sparse form.
struct SparseRun {
  int first, count;
  int64_t row0, rows;
};
// The range walked in runs of whole tables: a run takes tables while its stored rows fit stage_bytes
// (rows * row_bytes <= stage_bytes) and always holds at least one table, so a table larger than the
// bound is a run of its own.  The runs cover [0, count) in order; n_rows[k] >= 0.
std::vector<SparseRun> sparse_plan_runs(const int64_t* n_rows, int count, size_t row_bytes, size_t stage_bytes);

}  // namespace p2pmg
