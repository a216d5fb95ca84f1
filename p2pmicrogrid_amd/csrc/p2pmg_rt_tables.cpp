// p2pmg_rt_tables.cpp — the Q-tables as data: dense and sparse I/O, digests, copies, the shared-table
// deltas on this device, and the parity calls on single table rows (p2pmg_q_calls).
#include <algorithm>

#include "p2pmg_ctx.h"
#include "p2pmg_sparse.h"

using namespace p2pmg::rt;
using p2pmg::kQPad;

namespace {

int q_range_ok(p2pmg_ctx* c, int first, int count, const void* host, int dtype) {
  if (c && c->dqn) return 0;
  const int n_tables = c ? (int)c->n_tables : 0;
  if (!c || !host || first < 0 || count < 0 || first + count > n_tables) return 0;
  return dtype == P2PMG_Q_F64 || dtype == P2PMG_Q_F32;
}

}  // namespace

// ---- table digests: one pass of table_digest_kernel over tables [first, first + count) with the outputs
// of the call switched on.  Each returns `count == 0` before this is reached.  (Also what
// p2pmg_policy_set_capture, p2pmg_rt_policy.cpp, points at a policy-set slot.)
namespace p2pmg::rt {

int digest_range(p2pmg_ctx* c, int first, int count, const char* what) {
  if (!c) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_STATE, std::string(what) + ": DQN context has no Q-table");
  if (first < 0 || count < 0 || (size_t)first + (size_t)count > c->n_tables)
    return fail(c, P2PMG_E_INVALID, std::string(what) + ": bad table range");
  return P2PMG_OK;
}

p2pmg::TableDigestParams digest_params(p2pmg_ctx* c, int first, int count) {
  p2pmg::TableDigestParams p{};
  p.q = table_ptr(c, (size_t)first);
  p.n_states = c->n_states;
  p.n_actions = c->cfg.n_actions;
  p.count = count;
  p.bpt = p2pmg::table_digest_blocks(count, c->n_states);
  p.dword = c->n_states % 4 == 0 ? 1 : 0;  // every table's bytes then start 4-byte aligned
  return p;
}

}  // namespace p2pmg::rt

namespace {

// ---- sparse table checkpoints: the stored rows of tables [first, first + count) compacted on the device
// (count, offset and scatter passes of p2pmg_tables.hip), imported by a scatter, and one table copied
// over many.  Each returns `count == 0` before the device is reached.
static_assert(sizeof(long long) == sizeof(int64_t), "per-table totals travel as int64");

int sparse_range(p2pmg_ctx* c, int first, int count, const char* what) {
  RC_TRY(digest_range(c, first, count, what));
  if (c->n_states > 0x7FFFFFFFull)
    return fail(c, P2PMG_E_UNSUPPORTED, std::string(what) + ": row indices are int32 (n_states > 2^31 - 1)");
  return P2PMG_OK;
}

// the count and offset passes over the range; n_rows[count] on the host, *p what the scatter continues with
int sparse_count_pass(p2pmg_ctx* c, int first, int count, int64_t* n_rows, p2pmg::SparseParams* p) {
  *p = p2pmg::SparseParams{};
  p->q = table_ptr(c, (size_t)first);
  p->n_states = c->n_states;
  p->n_actions = c->cfg.n_actions;
  p->count = count;
  p2pmg::sparse_blocks(count, c->n_states, &p->bpt, &p->rpb);
  HIP_TRY(c, c->sp_blk.grow((size_t)count * p->bpt));
  HIP_TRY(c, c->sp_total.grow((size_t)count));
  p->blk = c->sp_blk;
  p->total = c->sp_total;
  HIP_TRY(c, p2pmg::launch_sparse_count(*p, c->cfg.q_dtype, c->stream));
  return download(c, {{n_rows, c->sp_total, (size_t)count * sizeof(int64_t)}});
}

// staging for the largest run, and every table's base inside its own run on the device
int sparse_stage(p2pmg_ctx* c, const std::vector<p2pmg::SparseRun>& runs, const int64_t* n_rows, int count,
                 size_t val_bytes) {
  int64_t most = 0;
  std::vector<long long> base((size_t)count);
  for (const p2pmg::SparseRun& r : runs) {
    most = std::max(most, r.rows);
    long long at = 0;
    for (int k = r.first; k < r.first + r.count; ++k) base[(size_t)k] = at, at += n_rows[k];
  }
  HIP_TRY(c, c->sp_rows.grow((size_t)most));
  HIP_TRY(c, c->sp_vals.grow((size_t)most * val_bytes));
  HIP_TRY(c, c->sp_base.grow((size_t)count));
  return upload(c, {{c->sp_base, base.data(), base.size() * sizeof(long long)}});  // synced: `base` goes out of scope
}

}  // namespace

extern "C" {

int p2pmg_zero_q(p2pmg_ctx* c) {
  if (!c) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_STATE, "zero_q: DQN context has no Q-table");
  HIP_TRY(c, hipMemsetAsync(c->q, 0, table_bytes(c, c->n_tables), c->stream));
  if (c->qdelta) HIP_TRY(c, hipMemsetAsync(c->qdelta, 0, p2pmg::kDeltaCopies * c->delta_n() * 8, c->stream));
  return P2PMG_OK;
}

int p2pmg_set_q(p2pmg_ctx* c, int first, int count, const void* host, int host_dtype) {
  if (!q_range_ok(c, first, count, host, host_dtype)) return fail(c, P2PMG_E_INVALID, "set_q: bad range/dtype");
  const int na = c->cfg.n_actions;
  const size_t hbytes = (size_t)count * c->n_states * na * (host_dtype == P2PMG_Q_F64 ? 8 : 4);
  DevBuf<char> staging;
  HIP_TRY(c, staging.alloc(hbytes));
  hipError_t e = hipMemcpyAsync(staging, host, hbytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = p2pmg::launch_q_pack(count, c->n_states, na, staging, table_ptr(c, (size_t)first), c->cfg.q_dtype, host_dtype,
                             c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("set_q: ") + hipGetErrorString(e));
  return P2PMG_OK;
}

int p2pmg_get_q(p2pmg_ctx* c, int first, int count, void* host, int host_dtype) {
  if (!q_range_ok(c, first, count, host, host_dtype)) return fail(c, P2PMG_E_INVALID, "get_q: bad range/dtype");
  const int na = c->cfg.n_actions;
  const size_t hbytes = (size_t)count * c->n_states * na * (host_dtype == P2PMG_Q_F64 ? 8 : 4);
  DevBuf<char> staging;
  HIP_TRY(c, staging.alloc(hbytes));
  hipError_t e = p2pmg::launch_q_unpack(count, c->n_states, na, table_ptr(c, (size_t)first), staging, c->cfg.q_dtype,
                                        host_dtype, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(host, staging, hbytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("get_q: ") + hipGetErrorString(e));
  return P2PMG_OK;
}

int p2pmg_table_stats(p2pmg_ctx* c, int first, int count, double* stats) {
  RC_TRY(digest_range(c, first, count, "table_stats"));
  if (count == 0) return P2PMG_OK;
  if (!stats) return fail(c, P2PMG_E_INVALID, "table_stats: null output");
  p2pmg::TableDigestParams p = digest_params(c, first, count);
  HIP_TRY(c, c->td_part.grow((size_t)count * p.bpt * P2PMG_TABLE_STATS));
  HIP_TRY(c, c->td_out.grow((size_t)count * P2PMG_TABLE_STATS));
  p.stat_part = c->td_part;
  p.stat_out = c->td_out;
  HIP_TRY(c, p2pmg::launch_table_digest(p, c->cfg.q_dtype, c->stream));
  return download(c, {{stats, c->td_out, (size_t)count * P2PMG_TABLE_STATS * sizeof(double)}});
}

int p2pmg_greedy_policy(p2pmg_ctx* c, int first, int count, uint8_t* policy) {
  RC_TRY(digest_range(c, first, count, "greedy_policy"));
  if (count == 0) return P2PMG_OK;
  if (!policy) return fail(c, P2PMG_E_INVALID, "greedy_policy: null output");
  const size_t bytes = (size_t)count * c->n_states;
  DevBuf<uint8_t> staging;
  HIP_TRY(c, staging.alloc(bytes));
  p2pmg::TableDigestParams p = digest_params(c, first, count);
  p.policy = staging;
  HIP_TRY(c, p2pmg::launch_table_digest(p, c->cfg.q_dtype, c->stream));
  return download(c, {{policy, staging, bytes}});
}

int p2pmg_policy_mark(p2pmg_ctx* c) {
  RC_TRY(digest_range(c, 0, 0, "policy_mark"));
  const bool fresh = !c->policy_snap;
  if (fresh && c->policy_snap.alloc(c->n_tables * c->n_states) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, P2PMG_E_NOMEM, "policy_mark: the policy snapshot ([n_tables][n_states] bytes)");
  }
  p2pmg::TableDigestParams p = digest_params(c, 0, (int)c->n_tables);
  p.policy = c->policy_snap;
  hipError_t e = p2pmg::launch_table_digest(p, c->cfg.q_dtype, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    if (fresh) c->policy_snap.release();  // no half-written first snapshot
    return fail(c, P2PMG_E_HIP, std::string("policy_mark: ") + hipGetErrorString(e));
  }
  return P2PMG_OK;
}

int p2pmg_policy_changes(p2pmg_ctx* c, int first, int count, int64_t* changed, int64_t* newly_visited, int remark) {
  RC_TRY(digest_range(c, first, count, "policy_changes"));
  if (!c->policy_snap) return fail(c, P2PMG_E_STATE, "policy_changes: p2pmg_policy_mark first");
  if (count == 0) return P2PMG_OK;
  if (!changed) return fail(c, P2PMG_E_INVALID, "policy_changes: null output");
  p2pmg::TableDigestParams p = digest_params(c, first, count);
  HIP_TRY(c, c->td_cpart.grow((size_t)count * p.bpt * 2));
  HIP_TRY(c, c->td_cout.grow((size_t)count * 2));
  p.snap = c->policy_snap.get() + (size_t)first * c->n_states;
  p.remark = remark ? 1 : 0;
  p.chg_part = c->td_cpart;
  p.chg_out = c->td_cout;
  HIP_TRY(c, p2pmg::launch_table_digest(p, c->cfg.q_dtype, c->stream));
  std::vector<long long> host((size_t)count * 2);
  RC_TRY(download(c, {{host.data(), c->td_cout, host.size() * sizeof(long long)}}));
  for (int k = 0; k < count; ++k) {
    changed[k] = host[2 * (size_t)k];
    if (newly_visited) newly_visited[k] = host[2 * (size_t)k + 1];
  }
  return P2PMG_OK;
}

int p2pmg_sparse_count(p2pmg_ctx* c, int first, int count, int64_t* n_rows) {
  RC_TRY(sparse_range(c, first, count, "sparse_count"));
  if (count == 0) return P2PMG_OK;
  if (!n_rows) return fail(c, P2PMG_E_INVALID, "sparse_count: null output");
  p2pmg::SparseParams p;
  return sparse_count_pass(c, first, count, n_rows, &p);
}

int p2pmg_get_q_sparse(p2pmg_ctx* c, int first, int count, int64_t capacity, int64_t* n_rows, int32_t* rows, void* values,
                       int host_dtype) {
  RC_TRY(sparse_range(c, first, count, "get_q_sparse"));
  if (count == 0) return P2PMG_OK;
  if (!n_rows || (host_dtype != P2PMG_Q_F64 && host_dtype != P2PMG_Q_F32))
    return fail(c, P2PMG_E_INVALID, "get_q_sparse: null n_rows or bad dtype");
  p2pmg::SparseParams p;
  RC_TRY(sparse_count_pass(c, first, count, n_rows, &p));
  int64_t total = 0;
  for (int k = 0; k < count; ++k) total += n_rows[k];
  if (total > capacity)
    return fail(c, P2PMG_E_INVALID, "get_q_sparse: " + std::to_string(total) + " stored rows exceed the capacity " +
                                        std::to_string(capacity) + " (n_rows is filled)");
  if (total == 0) return P2PMG_OK;
  if (!rows || !values) return fail(c, P2PMG_E_INVALID, "get_q_sparse: null output");
  const size_t val_bytes = p2pmg::sparse_row_bytes(p.n_actions, host_dtype) - sizeof(int32_t);
  const std::vector<p2pmg::SparseRun> runs =
      p2pmg::sparse_plan_runs(n_rows, count, p2pmg::sparse_row_bytes(p.n_actions, host_dtype), P2PMG_SPARSE_STAGE_BYTES);
  RC_TRY(sparse_stage(c, runs, n_rows, count, val_bytes));
  p.out_rows = c->sp_rows;
  p.out_vals = c->sp_vals;
  for (const p2pmg::SparseRun& r : runs) {
    if (r.rows == 0) continue;
    p2pmg::SparseParams pr = p;
    pr.q = table_ptr(c, (size_t)first + (size_t)r.first);
    pr.count = r.count;
    pr.blk = c->sp_blk.get() + (size_t)r.first * p.bpt;
    pr.base = c->sp_base.get() + r.first;
    HIP_TRY(c, p2pmg::launch_sparse_scatter(pr, c->cfg.q_dtype, host_dtype, c->stream));
    // synced: the next run reuses the staging
    RC_TRY(download(c, {{rows + r.row0, c->sp_rows, (size_t)r.rows * sizeof(int32_t)},
                        {static_cast<char*>(values) + (size_t)r.row0 * val_bytes, c->sp_vals, (size_t)r.rows * val_bytes}}));
  }
  return P2PMG_OK;
}

int p2pmg_set_q_sparse(p2pmg_ctx* c, int first, int count, const int64_t* n_rows, const int32_t* rows, const void* values,
                       int host_dtype, int zero_first) {
  RC_TRY(sparse_range(c, first, count, "set_q_sparse"));
  if (count == 0) return P2PMG_OK;
  if (!n_rows || (host_dtype != P2PMG_Q_F64 && host_dtype != P2PMG_Q_F32))
    return fail(c, P2PMG_E_INVALID, "set_q_sparse: null n_rows or bad dtype");
  int64_t total = 0;
  if (const char* bad = p2pmg::sparse_validate(n_rows, rows, count, c->n_states, &total))
    return fail(c, P2PMG_E_INVALID, std::string("set_q_sparse: ") + bad);
  if (total > 0 && !values) return fail(c, P2PMG_E_INVALID, "set_q_sparse: null values");
  if (zero_first) HIP_TRY(c, hipMemsetAsync(table_ptr(c, (size_t)first), 0, table_bytes(c, (size_t)count), c->stream));
  if (total > 0) {
    const int na = c->cfg.n_actions;
    const size_t val_bytes = p2pmg::sparse_row_bytes(na, host_dtype) - sizeof(int32_t);
    const std::vector<p2pmg::SparseRun> runs =
        p2pmg::sparse_plan_runs(n_rows, count, p2pmg::sparse_row_bytes(na, host_dtype), P2PMG_SPARSE_STAGE_BYTES);
    RC_TRY(sparse_stage(c, runs, n_rows, count, val_bytes));
    for (const p2pmg::SparseRun& r : runs) {
      if (r.rows == 0) continue;
      HIP_TRY(c, hipMemcpyAsync(c->sp_rows, rows + r.row0, (size_t)r.rows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, hipMemcpyAsync(c->sp_vals, static_cast<const char*>(values) + (size_t)r.row0 * val_bytes,
                                (size_t)r.rows * val_bytes, hipMemcpyHostToDevice, c->stream));
      p2pmg::SparseImportParams ip{};
      ip.q = table_ptr(c, (size_t)first + (size_t)r.first);
      ip.n_states = c->n_states;
      ip.n_actions = na;
      ip.count = r.count;
      ip.total = r.rows;
      ip.base = c->sp_base.get() + r.first;
      ip.rows = c->sp_rows;
      ip.vals = c->sp_vals;
      HIP_TRY(c, p2pmg::launch_sparse_import(ip, c->cfg.q_dtype, host_dtype, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));  // the next run reuses the staging
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_copy_q(p2pmg_ctx* c, int src, int dst_first, int dst_count) {
  RC_TRY(sparse_range(c, dst_first, dst_count, "copy_q"));
  if (dst_count == 0) return P2PMG_OK;
  if (src < 0 || (size_t)src >= c->n_tables || (src >= dst_first && src < dst_first + dst_count))
    return fail(c, P2PMG_E_INVALID, "copy_q: the source is no table, or lies inside the destination range");
  // the source over the first destination, then the copies made so far over as many more: ceil(log2
  // (dst_count)) + 1 device-to-device copies, each one contiguous run of whole tables
  const size_t bytes = table_bytes(c);
  char* dst = table_ptr(c, (size_t)dst_first);
  HIP_TRY(c, hipMemcpyAsync(dst, table_ptr(c, (size_t)src), bytes, hipMemcpyDeviceToDevice, c->stream));
  for (size_t done = 1; done < (size_t)dst_count;) {
    const size_t k = std::min(done, (size_t)dst_count - done);
    HIP_TRY(c, hipMemcpyAsync(dst + done * bytes, dst, k * bytes, hipMemcpyDeviceToDevice, c->stream));
    done += k;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_apply_q_delta(p2pmg_ctx* c) {
  if (!c) return P2PMG_E_INVALID;
  if (!c->qdelta) return fail(c, P2PMG_E_STATE, "apply_q_delta: context has no shared table");
  HIP_TRY(c, p2pmg::launch_fold_delta(c->qdelta, c->delta_n(), c->stream));
  HIP_TRY(c, p2pmg::launch_apply_delta(c->q, c->qdelta, c->delta_n(), c->cfg.q_dtype, c->stream));
  return P2PMG_OK;
}

int p2pmg_get_q_delta(p2pmg_ctx* c, int64_t* host) {
  if (!c || !host) return P2PMG_E_INVALID;
  if (!c->qdelta) return fail(c, P2PMG_E_STATE, "get_q_delta: context has no shared table");
  const int na = c->cfg.n_actions;
  std::vector<long long> h(c->delta_n());
  HIP_TRY(c, p2pmg::launch_fold_delta(c->qdelta, c->delta_n(), c->stream));
  RC_TRY(download(c, {{h.data(), c->qdelta, h.size() * 8}}));
  for (size_t r = 0; r < c->n_tables * c->n_states; ++r)  // rows of every table, in table order
    for (int k = 0; k < na; ++k) host[r * na + k] = h[r * kQPad + k];
  return P2PMG_OK;
}

int p2pmg_set_q_delta(p2pmg_ctx* c, const int64_t* host) {
  if (!c || !host) return P2PMG_E_INVALID;
  if (!c->qdelta) return fail(c, P2PMG_E_STATE, "set_q_delta: context has no shared table");
  const int na = c->cfg.n_actions;
  std::vector<long long> h(c->delta_n(), 0);
  for (size_t r = 0; r < c->n_tables * c->n_states; ++r)
    for (int k = 0; k < na; ++k) h[r * kQPad + k] = host[r * na + k];
  HIP_TRY(c, hipMemsetAsync(c->qdelta, 0, p2pmg::kDeltaCopies * h.size() * 8, c->stream));
  return upload(c, {{c->qdelta, h.data(), h.size() * 8}});
}

int p2pmg_q_calls(p2pmg_ctx* c, int n, const int32_t* agents, const float* s_obs, const uint8_t* codes,
                  const float* rewards, const float* ns_obs, int train, int32_t* actions_out, double* q_out) {
  if (!c || n < 0 || !agents || !s_obs || !codes || !actions_out || !q_out) return P2PMG_E_INVALID;
  if (train && (!rewards || !ns_obs)) return fail(c, P2PMG_E_INVALID, "q_calls: train needs rewards and ns_obs");
  if (c->dqn) return fail(c, P2PMG_E_STATE, "q_calls: DQN context has no Q-table");
  if (c->cfg.n_actions != 3) return fail(c, P2PMG_E_UNSUPPORTED, "q_calls: the kernels act on 3 actions (this context only holds tables)");
  for (int k = 0; k < n; ++k)
    if (agents[k] < 0 || (size_t)agents[k] >= c->n_tables) return fail(c, P2PMG_E_INVALID, "q_calls: agent out of range");
  if (n == 0) return P2PMG_OK;
  // one staging block: agents | s_obs | ns_obs | rewards | codes | actions | q_out
  const size_t nb = (size_t)n;
  const size_t off_s = 0, off_ns = off_s + 16 * nb, off_r = off_ns + 16 * nb, off_a = off_r + 4 * nb,
               off_act = off_a + 4 * nb, off_q = ((off_act + 4 * nb + 7) / 8) * 8, off_c = off_q + 8 * nb,
               total = off_c + nb;
  DevBuf<char> d;
  HIP_TRY(c, d.alloc(total));
  hipError_t e = hipMemcpyAsync(d + off_s, s_obs, 16 * nb, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && train) e = hipMemcpyAsync(d + off_ns, ns_obs, 16 * nb, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && train) e = hipMemcpyAsync(d + off_r, rewards, 4 * nb, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + off_a, agents, 4 * nb, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + off_c, codes, nb, hipMemcpyHostToDevice, c->stream);
  const p2pmg_config& g = c->cfg;
  p2pmg::QCallParams p{n, train ? 1 : 0, g.q_dtype, reinterpret_cast<const int32_t*>(d + off_a),
                       reinterpret_cast<const float*>(d + off_s), reinterpret_cast<const uint8_t*>(d + off_c),
                       reinterpret_cast<const float*>(d + off_r), reinterpret_cast<const float*>(d + off_ns),
                       reinterpret_cast<int32_t*>(d + off_act), reinterpret_cast<double*>(d + off_q), c->q,
                       (uint32_t)c->n_states, g.n_time_states, g.n_temp_states, g.n_balance_states, g.n_p2p_states,
                       c->learn};
  if (e == hipSuccess) e = p2pmg::launch_q_calls(p, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(actions_out, d + off_act, 4 * nb, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(q_out, d + off_q, 8 * nb, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("q_calls: ") + hipGetErrorString(e));
  return P2PMG_OK;
}

}  // extern "C"
