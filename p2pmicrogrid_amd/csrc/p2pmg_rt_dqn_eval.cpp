// p2pmg_rt_dqn_eval.cpp — DQN evaluation: the context's policy set (M frozen networks and an agent ->
// network map) and the one-launch greedy episode, dqn_greedy_episode_kernel, on the policy set or on the
// learner's own online / target networks.  Nothing here writes a weight array, an Adam step count, a
// replay ring or the replay-code state.
#include <algorithm>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;

extern "C" {

int p2pmg_dqn_set_policy_nets(p2pmg_ctx* c, int count, const float* weights, const int32_t* net_of) {
  RC_TRY(dqn_ready(c, "dqn_set_policy_nets"));
  if (count < 0) return fail(c, P2PMG_E_INVALID, "dqn_set_policy_nets: negative count");
  if (count == 0) {
    c->d_pol.release();
    c->d_pol_map.release();
    c->h_pol_map.clear();
    c->pol_count = 0;
    return P2PMG_OK;
  }
  if (!weights) return fail(c, P2PMG_E_INVALID, "dqn_set_policy_nets: null weights");
  // the whole map on the host first: nothing is uploaded, and the current set stays, unless it is valid
  std::vector<int32_t> map((size_t)c->A);
  if (net_of) {
    for (int a = 0; a < c->A; ++a) {
      if (net_of[a] < 0 || net_of[a] >= count)
        return fail(c, P2PMG_E_INVALID, "dqn_set_policy_nets: net_of[" + std::to_string(a) + "] = " +
                                            std::to_string(net_of[a]) + " outside [0, " + std::to_string(count) + ")");
      map[(size_t)a] = net_of[a];
    }
  } else if (count == c->N) {
    for (int a = 0; a < c->A; ++a) map[(size_t)a] = a % count;  // role i of every scenario
  } else if (count == c->A) {
    for (int a = 0; a < c->A; ++a) map[(size_t)a] = a;
  } else if (count == 1) {
    for (int a = 0; a < c->A; ++a) map[(size_t)a] = 0;
  } else {
    return fail(c, P2PMG_E_INVALID, "dqn_set_policy_nets: without net_of, count must be N, A or 1");
  }
  const size_t NS = p2pmg::kNetStride;
  DevBuf<float> nets;
  DevBuf<int32_t> dmap;
  HIP_TRY(c, nets.alloc((size_t)count * NS));
  HIP_TRY(c, dmap.alloc((size_t)c->A));
  HIP_TRY(c, hipMemsetAsync(nets.get(), 0, (size_t)count * NS * 4, c->stream));
  HIP_TRY(c, hipMemcpy2DAsync(nets.get(), NS * 4, weights, p2pmg::kDqnParams * 4, p2pmg::kDqnParams * 4, (size_t)count,
                              hipMemcpyHostToDevice, c->stream));
  RC_TRY(upload(c, {{dmap.get(), map.data(), map.size() * sizeof(int32_t)}}));  // synced: the caller's arrays are free
  c->d_pol = std::move(nets);  // the previous set, if any, is freed here, after the stream has drained
  c->d_pol_map = std::move(dmap);
  c->h_pol_map = std::move(map);
  c->pol_count = count;
  return P2PMG_OK;
}

int p2pmg_dqn_get_policy_nets(p2pmg_ctx* c, int* count, float* weights, int32_t* net_of) {
  RC_TRY(dqn_ready(c, "dqn_get_policy_nets"));
  if (count) *count = c->pol_count;
  if (c->pol_count == 0) return P2PMG_OK;
  if (net_of) std::copy(c->h_pol_map.begin(), c->h_pol_map.end(), net_of);
  if (weights) {
    HIP_TRY(c, hipMemcpy2DAsync(weights, p2pmg::kDqnParams * 4, c->d_pol.get(), p2pmg::kNetStride * 4,
                                p2pmg::kDqnParams * 4, (size_t)c->pol_count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return P2PMG_OK;
}

int p2pmg_dqn_run_greedy(p2pmg_ctx* c, int source, int record) {
  RC_TRY(dqn_ready(c, "dqn_run_greedy"));
  constexpr int kRecords = P2PMG_REC_REWARD | P2PMG_REC_COST | P2PMG_REC_GRID | P2PMG_REC_P2P | P2PMG_REC_TEMP |
                           P2PMG_REC_ACTION;
  if (record & ~kRecords)
    return fail(c, P2PMG_E_INVALID, "dqn_run_greedy: records are reward, cost, grid, p2p, temp and action (a greedy "
                                    "episode trains nothing: no loss)");
  if (source != P2PMG_DQN_ONLINE && source != P2PMG_DQN_TARGET && source != P2PMG_DQN_POLICY_SET)
    return fail(c, P2PMG_E_INVALID, "dqn_run_greedy: source must be P2PMG_DQN_ONLINE, P2PMG_DQN_TARGET or P2PMG_DQN_POLICY_SET");
  if (source == P2PMG_DQN_POLICY_SET && c->pol_count == 0)
    return fail(c, P2PMG_E_STATE, "dqn_run_greedy: p2pmg_dqn_set_policy_nets first");
  if (!c->have_env || !c->have_prof || !c->have_params)
    return fail(c, P2PMG_E_STATE, "dqn_run_greedy: env, profiles and agent params must be set first");
  RC_TRY(ensure_records(c, record));
  const p2pmg_episode_args args{P2PMG_MODE_GREEDY, P2PMG_RNG_PHILOX, 0, record, 0.0, 0, 0};
  p2pmg::DqnEvalParams d{};
  d.e = episode_params(c, &args);
  if (source == P2PMG_DQN_POLICY_SET) {
    d.nets = c->d_pol;
    d.net_of = c->d_pol_map;
  } else {
    d.nets = dqn_array(c, source);
    d.net_of = c->dqn_roles ? c->d_role_map.get() : nullptr;  // a role context: agent a on network a % N
    d.one_net = c->n_nets == 1 ? 1 : 0;
  }
  d.ep_acc = c->d_ep_acc;
  d.penw = c->d_penw;
  Timed tm;
  RC_TRY(begin_timed(c, false, true, &tm));
  const hipError_t e = p2pmg::launch_dqn_greedy_episode(d, c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("dqn greedy episode launch: ") + hipGetErrorString(e));
  RC_TRY(end_timed(c, tm, true));
  finish_launch(c, tm, "dqn_greedy_episode_kernel<" + std::to_string(c->N) + ">", record, 0, 0);
  return P2PMG_OK;
}

}  // extern "C"
