// p2pmg_sparse.cpp — see p2pmg_sparse.h.  No HIP call and no device.
#include "p2pmg_sparse.h"

namespace p2pmg {

const char* sparse_validate(const int64_t* n_rows, const int32_t* rows, int count, size_t n_states, int64_t* total) {
  if (!n_rows || count < 0 || n_states > 0x7FFFFFFFull) return "bad arguments";
  int64_t at = 0;  // <= count * n_states < 2^62
  for (int k = 0; k < count; ++k) {
    const int64_t m = n_rows[k];
    if (m < 0 || m > (int64_t)n_states) return "n_rows outside [0, n_states]";
    if (m > 0 && !rows) return "null rows";
    int64_t prev = -1;
    for (int64_t i = 0; i < m; ++i) {
      const int64_t r = rows[at + i];
      if (r < 0 || r >= (int64_t)n_states) return "row index outside [0, n_states)";
      if (r <= prev) return "row indices not strictly ascending inside a table";
      prev = r;
    }
    at += m;
  }
  *total = at;
  return nullptr;
}

std::vector<SparseRun> sparse_plan_runs(const int64_t* n_rows, int count, size_t row_bytes, size_t stage_bytes) {
  std::vector<SparseRun> runs;
  const int64_t cap = (int64_t)(stage_bytes / (row_bytes ? row_bytes : 1));  // rows a run may hold
  int64_t row0 = 0;
  for (int k = 0; k < count;) {
    SparseRun r{k, 1, row0, n_rows[k]};
    for (++k; k < count && n_rows[k] <= cap - r.rows; ++k) {  // cap - r.rows < 0 after an oversized first table
      r.rows += n_rows[k];
      ++r.count;
    }
    row0 += r.rows;
    runs.push_back(r);
  }
  return runs;
}

}  // namespace p2pmg
