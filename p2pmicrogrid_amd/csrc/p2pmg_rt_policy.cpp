// p2pmg_rt_policy.cpp — the policy set of a tabular context (M packed byte policies and an agent -> policy
// map beside the tables), its capture from the tables on the device, and the one-launch greedy episode that
// acts from it, policy_episode_kernel.  Nothing here writes a table, a delta, the policy-mark snapshot or the
// replay-code state; no other unit reads or writes the set.
#include <algorithm>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;

namespace {

int tabular_ctx(p2pmg_ctx* c, const char* what) {
  if (!c) return P2PMG_E_INVALID;
  if (c->dqn) return fail(c, P2PMG_E_STATE, std::string(what) + ": DQN context (p2pmg_dqn_set_policy_nets holds its policy set)");
  return P2PMG_OK;
}

int run_policy_impl(p2pmg_ctx* c, int record, int flags) {
  RC_TRY(tabular_ctx(c, "run_policy"));
  if (c->cfg.n_actions != 3)
    return fail(c, P2PMG_E_UNSUPPORTED, "run_policy: the kernels act on 3 actions (this context only holds tables)");
  if (c->pset_count == 0) return fail(c, P2PMG_E_STATE, "run_policy: p2pmg_set_policy_set first");
  if (!c->have_env || !c->have_prof || !c->have_params)
    return fail(c, P2PMG_E_STATE, "run_policy: env, profiles and agent params must be set first");
  constexpr int kRecords = P2PMG_REC_REWARD | P2PMG_REC_COST | P2PMG_REC_GRID | P2PMG_REC_P2P | P2PMG_REC_TEMP |
                           P2PMG_REC_ACTION | P2PMG_REC_INDEX;
  if (record & ~kRecords) return fail(c, P2PMG_E_INVALID, "run_policy: records are every P2PMG_REC_* but LOSS");
  if (flags & ~P2PMG_FLAG_TILE_KERNEL) return fail(c, P2PMG_E_INVALID, "run_policy_ex: flags are 0 or P2PMG_FLAG_TILE_KERNEL");
  RC_TRY(ensure_records(c, record));
  c->chain_n = 0;  // p2pmg_get_episode_rewards covers p2pmg_run_episodes calls only
  p2pmg_episode_args args{};
  args.mode = P2PMG_MODE_GREEDY;
  args.record = record;
  p2pmg::PolicyParams pp{};
  pp.e = episode_params(c, &args);
  pp.pol = c->pset;
  pp.pol_of = c->pset_map;
  const bool regs = c->N <= 8 || c->N == 16;
  const bool tile = (flags & P2PMG_FLAG_TILE_KERNEL) != 0 || !regs;
  Timed tm;
  RC_TRY(begin_timed(c, false, true, &tm));
  const hipError_t e = p2pmg::launch_policy_episode(pp, tile ? 1 : 0, c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("policy episode launch: ") + hipGetErrorString(e));
  RC_TRY(end_timed(c, tm, true));
  finish_launch(c, tm,
                "policy_episode_kernel<" + std::to_string(c->N) +
                    (tile ? ",tile" + std::to_string(p2pmg::general_tile_cap(c->N)) : "") + ",R1=" +
                    std::to_string(c->R + 1) + (c->battery ? ",battery>" : ">"),
                record, 0, 0);
  return P2PMG_OK;
}

}  // namespace

extern "C" {

int p2pmg_set_policy_set(p2pmg_ctx* c, int count, const uint8_t* policies, const int32_t* policy_of) {
  RC_TRY(tabular_ctx(c, "set_policy_set"));
  if (count == 0) {
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // a launch that reads the set may still run
    c->pset.release();
    c->pset_map.release();
    c->h_pset_map.clear();
    c->pset_count = 0;
    return P2PMG_OK;
  }
  // the whole input on the host first: nothing is uploaded, and the current set stays, unless it is valid
  std::vector<int32_t> map(count > 0 ? (size_t)c->A : 0);
  std::string why;
  const int rc = p2pmg::validate_policy_set(count, policies, policy_of, c->n_states, c->cfg.n_actions, c->N, c->S,
                                            map.data(), &why);
  if (rc != P2PMG_OK) return fail(c, rc, why);
  const size_t bytes = (size_t)count * c->n_states;
  DevBuf<uint8_t> set;
  DevBuf<int32_t> dmap;
  if (set.alloc(bytes) != hipSuccess || dmap.alloc((size_t)c->A) != hipSuccess) {
    (void)hipGetLastError();  // the set the context held stays as it was
    return fail(c, P2PMG_E_NOMEM, "set_policy_set: the policy set (" + std::to_string(bytes) + " + " +
                                      std::to_string((size_t)c->A * sizeof(int32_t)) + " bytes on the device)");
  }
  if (policies) HIP_TRY(c, hipMemcpyAsync(set.get(), policies, bytes, hipMemcpyHostToDevice, c->stream));
  else HIP_TRY(c, hipMemsetAsync(set.get(), P2PMG_POLICY_UNVISITED, bytes, c->stream));
  RC_TRY(upload(c, {{dmap.get(), map.data(), map.size() * sizeof(int32_t)}}));  // synced: the caller's arrays are free
  c->pset = std::move(set);  // the previous set, if any, is freed here, after the stream has drained
  c->pset_map = std::move(dmap);
  c->h_pset_map = std::move(map);
  c->pset_count = count;
  return P2PMG_OK;
}

int p2pmg_get_policy_set(p2pmg_ctx* c, int* count, uint8_t* policies, int32_t* policy_of) {
  RC_TRY(tabular_ctx(c, "get_policy_set"));
  if (count) *count = c->pset_count;
  if (c->pset_count == 0) return P2PMG_OK;
  if (policy_of) std::copy(c->h_pset_map.begin(), c->h_pset_map.end(), policy_of);
  if (policies) return download(c, {{policies, c->pset, (size_t)c->pset_count * c->n_states}});
  return P2PMG_OK;
}

int p2pmg_policy_set_capture(p2pmg_ctx* c, int first_table, int count, int first_slot) {
  RC_TRY(tabular_ctx(c, "policy_set_capture"));
  if (c->pset_count == 0) return fail(c, P2PMG_E_STATE, "policy_set_capture: p2pmg_set_policy_set first");
  RC_TRY(digest_range(c, first_table, count, "policy_set_capture"));
  if (first_slot < 0 || (long long)first_slot + count > c->pset_count)
    return fail(c, P2PMG_E_INVALID, "policy_set_capture: bad slot range");
  if (count == 0) return P2PMG_OK;
  // the digest pass of p2pmg_greedy_policy with the set's slots as its output: same kernel, same bytes
  p2pmg::TableDigestParams p = digest_params(c, first_table, count);
  p.policy = c->pset.get() + (size_t)first_slot * c->n_states;
  HIP_TRY(c, p2pmg::launch_table_digest(p, c->cfg.q_dtype, c->stream));
  return P2PMG_OK;
}

int p2pmg_run_policy(p2pmg_ctx* c, int record) { return run_policy_impl(c, record, 0); }

int p2pmg_run_policy_ex(p2pmg_ctx* c, int record, int flags) { return run_policy_impl(c, record, flags); }

}  // extern "C"
