// sparse_check.cpp — stand-alone check of the host side of the sparse table checkpoints
// (csrc/p2pmg_sparse.cpp): the validation of an uploaded sparse form and the walk of a table range in
// staging runs.  No HIP device is taken.  Every array handed to the code under test is a heap block of
// exactly the size the interface promises to read, so that under -fsanitize=address,undefined a read past
// it, or past the point where the check must stop, is a report.  Built and run by
// tests/test_cpu_sparse_tables.py; exits 0 and prints "ok <n>" when every case holds.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "p2pmg.h"
#include "p2pmg_sparse.h"

using namespace p2pmg;

static int failures = 0, checks = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    ++checks;                                                        \
    if (!(cond)) {                                                   \
      ++failures;                                                    \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
    }                                                                \
  } while (0)

// exact-size heap copies (a vector's capacity may exceed its size)
template <typename T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size()]);
  if (!v.empty()) std::memcpy(p.get(), v.data(), v.size() * sizeof(T));
  return p;
}

// null: accepted; *total as the check left it
static const char* validate(const std::vector<int64_t>& n_rows, const std::vector<int32_t>& rows, size_t n_states,
                            int64_t* total) {
  const auto n = exact(n_rows);
  const auto r = exact(rows);
  return sparse_validate(n.get(), rows.empty() ? nullptr : r.get(), (int)n_rows.size(), n_states, total);
}

static std::vector<SparseRun> plan(const std::vector<int64_t>& n_rows, size_t row_bytes, size_t stage) {
  const auto n = exact(n_rows);
  return sparse_plan_runs(n.get(), (int)n_rows.size(), row_bytes, stage);
}

// the runs cover [0, count) in order, whole tables, each within the bound or a single table
static bool covers(const std::vector<SparseRun>& runs, const std::vector<int64_t>& n_rows, size_t row_bytes, size_t stage) {
  int k = 0;
  int64_t row0 = 0;
  for (size_t i = 0; i < runs.size(); ++i) {
    const SparseRun& r = runs[i];
    if (r.first != k || r.count < 1 || r.row0 != row0) return false;
    int64_t rows = 0;
    for (int j = 0; j < r.count; ++j) rows += n_rows[(size_t)(k + j)];
    if (rows != r.rows) return false;
    if (r.count > 1 && (uint64_t)rows * row_bytes > stage) return false;
    // greedy: the next table would not have fitted
    if (i + 1 < runs.size() && (uint64_t)(rows + n_rows[(size_t)(k + r.count)]) * row_bytes <= stage) return false;
    k += r.count;
    row0 += rows;
  }
  return k == (int)n_rows.size();
}

static bool says(const char* msg, const char* what) { return msg && std::strstr(msg, what); }

int main() {
  int64_t total = -7;
  {  // accepted forms
    CHECK(!validate({}, {}, 10, &total) && total == 0);
    CHECK(!validate({0, 0, 0}, {}, 10, &total) && total == 0);
    CHECK(!validate({3, 0, 2}, {0, 4, 9, 0, 9}, 10, &total) && total == 5);  // a table may restart below the one before
    CHECK(!validate({1, 1}, {9, 9}, 10, &total) && total == 2);              // the same index in two tables
    std::vector<int32_t> all(10);
    for (int i = 0; i < 10; ++i) all[(size_t)i] = i;
    CHECK(!validate({10}, all, 10, &total) && total == 10);                  // n_rows == n_states
    CHECK(!validate({1}, {0x7FFFFFFE}, 0x7FFFFFFFull, &total) && total == 1);
  }
  {  // refused forms: the message names the rule
    total = -7;
    CHECK(says(validate({2}, {5, 3}, 10, &total), "ascending") && total == -7);    // unsorted
    CHECK(says(validate({2}, {4, 4}, 10, &total), "ascending"));                   // duplicated
    CHECK(says(validate({2, 2}, {1, 2, 3, 3}, 10, &total), "ascending"));          // ... in a later table
    CHECK(says(validate({1}, {-1}, 10, &total), "outside"));                       // negative
    CHECK(says(validate({1}, {10}, 10, &total), "outside"));                       // == n_states
    CHECK(says(validate({2}, {0, 0x7FFFFFFF}, 10, &total), "outside"));
    CHECK(says(validate({1}, {INT32_MIN}, 10, &total), "outside"));
    // n_rows out of range: nothing of `rows` at or after that table may be read (there is none to read)
    CHECK(says(validate({-1}, {}, 10, &total), "n_rows"));
    CHECK(says(validate({11}, {0}, 10, &total), "n_rows"));
    CHECK(says(validate({1, 11}, {3}, 10, &total), "n_rows"));
    CHECK(says(validate({INT64_MAX}, {0}, 10, &total), "n_rows"));
    CHECK(says(validate({1, INT64_MIN}, {0}, 10, &total), "n_rows"));
    CHECK(says(validate({2}, {}, 10, &total), "null rows"));
    CHECK(sparse_validate(nullptr, nullptr, 1, 10, &total) != nullptr);
    const int64_t one = 0;
    CHECK(sparse_validate(&one, nullptr, -1, 10, &total) != nullptr);
    CHECK(sparse_validate(&one, nullptr, 1, 0x80000000ull, &total) != nullptr);
  }
  {  // run planning
    const size_t rb = sparse_row_bytes(3, P2PMG_Q_F64);
    CHECK(rb == 28 && sparse_row_bytes(3, P2PMG_Q_F32) == 16 && sparse_row_bytes(2, P2PMG_Q_F64) == 20);
    CHECK(plan({}, rb, 1000).empty());
    std::vector<SparseRun> r = plan({0, 0, 0}, rb, 1000);
    CHECK(r.size() == 1 && r[0].first == 0 && r[0].count == 3 && r[0].rows == 0 && r[0].row0 == 0);
    r = plan({10, 10, 10, 10}, 28, 28 * 20);  // exactly two tables fit
    CHECK(r.size() == 2 && r[0].count == 2 && r[1].first == 2 && r[1].count == 2 && r[1].row0 == 20 && r[1].rows == 20);
    r = plan({10, 10, 10, 10}, 28, 28 * 20 - 1);  // one byte short: one table per run
    CHECK(r.size() == 4 && r[3].row0 == 30);
    r = plan({100, 1, 1}, 28, 28 * 20);  // a table larger than the bound is a run of its own
    CHECK(r.size() == 2 && r[0].count == 1 && r[0].rows == 100 && r[1].first == 1 && r[1].count == 2 && r[1].row0 == 100);
    r = plan({1, 100, 1}, 28, 28 * 20);
    CHECK(r.size() == 3 && r[1].rows == 100 && r[2].row0 == 101);
    r = plan({5, 0, 0, 5}, 28, 0);  // no room at all: still one table at least, and an oversized table stays alone
    CHECK(r.size() == 3 && r[0].count == 1 && r[1].count == 2 && r[1].rows == 0 && r[2].first == 3 && r[2].row0 == 5);
    // the headline shapes: 160000-row tables, one full, under the library's bound
    const std::vector<int64_t> full = {140000, 0, 160000};  // 300000 rows x 28 B > 8 MiB
    r = plan(full, rb, P2PMG_SPARSE_STAGE_BYTES);
    CHECK(r.size() == 2 && r[0].count == 2 && r[1].rows == 160000 && covers(r, full, rb, P2PMG_SPARSE_STAGE_BYTES));
    // many shapes against the properties
    uint64_t s = 12345;
    for (int it = 0; it < 200; ++it) {
      std::vector<int64_t> n;
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      const int count = 1 + (int)((s >> 33) % 40);
      for (int k = 0; k < count; ++k) {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        n.push_back((s >> 60) < 3 ? 0 : (int64_t)((s >> 33) % 3000));
      }
      const size_t stage = 28 * (size_t)(1 + (s >> 40) % 6000);
      CHECK(covers(plan(n, 28, stage), n, 28, stage));
    }
    // counts near the top of the range do not overflow the running sum
    r = plan({INT64_MAX / 64, INT64_MAX / 64, 5}, 28, P2PMG_SPARSE_STAGE_BYTES);
    CHECK(r.size() == 3 && r[2].row0 == 2 * (INT64_MAX / 64));
  }
  if (failures) return 1;
  std::printf("ok %d\n", checks);
  return 0;
}
