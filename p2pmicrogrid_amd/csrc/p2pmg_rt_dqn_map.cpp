// p2pmg_rt_dqn_map.cpp — the DQN policy map: one pass of dqn_map_kernel over networks
// [first, first + count) of one weight array and the states of the grid, with the outputs of the call
// switched on.
#include <algorithm>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;

namespace {

int map_upload_grid(p2pmg_ctx* c, const uint32_t n[4], std::vector<float> axes) {
  HIP_TRY(c, c->map_axes.alloc(axes.size()));
  RC_TRY(upload(c, {{c->map_axes, axes.data(), axes.size() * sizeof(float)}}));
  for (int k = 0; k < 4; ++k) c->map_n[k] = n[k];
  c->map_G = (size_t)n[0] * n[1] * n[2] * n[3];
  c->h_map_axes = std::move(axes);
  c->map_snap.release();  // a snapshot belongs to the grid it was taken on
  return P2PMG_OK;
}

// the table shape with each axis at its bins' centres (formed in f64, cast to f32): state g of the map is
// then the state of row g of a table's packed policy
int map_default_grid(p2pmg_ctx* c, const char* what) {
  const int K[4] = {c->cfg.n_time_states, c->cfg.n_temp_states, c->cfg.n_balance_states, c->cfg.n_p2p_states};
  if (K[0] < 1 || K[1] < 3 || K[2] < 1 || K[3] < 1)
    return fail(c, P2PMG_E_INVALID, std::string(what) + ": the default grid needs n_temp_states >= 3 (p2pmg_dqn_set_grid)");
  if ((double)K[0] * K[1] * K[2] * K[3] > 2147483647.0)
    return fail(c, P2PMG_E_INVALID, std::string(what) + ": more than 2^31 - 1 grid states");
  std::vector<float> ax;
  for (int k = 0; k < K[0]; ++k) ax.push_back((float)((k + 0.5) / K[0]));
  for (int k = 0; k < K[1]; ++k) ax.push_back((float)(2.0 * (k - 0.5) / (K[1] - 2) - 1.0));
  for (int k = 0; k < K[2]; ++k) ax.push_back((float)(2.0 * (k + 0.5) / K[2] - 1.0));
  for (int k = 0; k < K[3]; ++k) ax.push_back((float)(2.0 * (k + 0.5) / K[3] - 1.0));
  const uint32_t n[4] = {(uint32_t)K[0], (uint32_t)K[1], (uint32_t)K[2], (uint32_t)K[3]};
  return map_upload_grid(c, n, std::move(ax));
}

int map_range(p2pmg_ctx* c, int which, int first, int count, const char* what) {
  RC_TRY(dqn_ready(c, what));
  if (which != P2PMG_DQN_ONLINE && which != P2PMG_DQN_TARGET)
    return fail(c, P2PMG_E_INVALID, std::string(what) + ": which must be P2PMG_DQN_ONLINE or P2PMG_DQN_TARGET");
  if (first < 0 || count < 0 || (size_t)first + (size_t)count > (size_t)c->n_nets)
    return fail(c, P2PMG_E_INVALID, std::string(what) + ": bad network range");
  return P2PMG_OK;
}

// networks [first, first + count) of `which` over the states [g0, g0 + gn) of the grid in use
p2pmg::DqnMapParams map_params(p2pmg_ctx* c, int which, int first, int count, size_t g0, size_t gn) {
  p2pmg::DqnMapParams p{};
  p.theta = dqn_array(c, which) + (size_t)first * p2pmg::kNetStride;
  p.count = count;
  for (int k = 0; k < 4; ++k) p.n[k] = c->map_n[k];
  p.axes = c->map_axes;
  p.g_begin = (uint32_t)g0;
  p.g_count = (uint32_t)gn;
  p.bpn = p2pmg::dqn_map_blocks(count, p.g_count);
  p.dword = gn % 4 == 0 ? 1 : 0;  // every network's bytes then start 4-byte aligned
  return p;
}

int map_scratch(p2pmg_ctx* c, p2pmg::DqnMapParams& p) {
  HIP_TRY(c, c->map_part.grow((size_t)p.count * p.bpn));
  p.part = c->map_part;
  return P2PMG_OK;
}

}  // namespace

extern "C" {

int p2pmg_dqn_set_grid(p2pmg_ctx* c, const int32_t* n, const float* time, const float* temp, const float* balance,
                       const float* p2p) {
  RC_TRY(dqn_ready(c, "dqn_set_grid"));
  const float* ax[4] = {time, temp, balance, p2p};
  if (!time && !temp && !balance && !p2p) return map_default_grid(c, "dqn_set_grid");
  if (!n || !time || !temp || !balance || !p2p) return fail(c, P2PMG_E_INVALID, "dqn_set_grid: four axes and n, or none");
  double G = 1.0;
  for (int k = 0; k < 4; ++k) {
    if (n[k] < 1) return fail(c, P2PMG_E_INVALID, "dqn_set_grid: every axis needs at least one value");
    G *= n[k];
  }
  if (G > 2147483647.0) return fail(c, P2PMG_E_INVALID, "dqn_set_grid: more than 2^31 - 1 grid states");
  std::vector<float> v;
  uint32_t un[4];
  for (int k = 0; k < 4; ++k) {
    un[k] = (uint32_t)n[k];
    v.insert(v.end(), ax[k], ax[k] + n[k]);
  }
  return map_upload_grid(c, un, std::move(v));
}

int p2pmg_dqn_get_grid(p2pmg_ctx* c, int32_t* n, float* axes) {
  RC_TRY(dqn_ready(c, "dqn_get_grid"));
  if (!n) return fail(c, P2PMG_E_INVALID, "dqn_get_grid: null output");
  if (!c->map_axes) RC_TRY(map_default_grid(c, "dqn_get_grid"));
  for (int k = 0; k < 4; ++k) n[k] = (int32_t)c->map_n[k];
  if (axes) std::copy(c->h_map_axes.begin(), c->h_map_axes.end(), axes);
  return P2PMG_OK;
}

int p2pmg_dqn_policy_map(p2pmg_ctx* c, int which, int first, int count, uint8_t* policy, float* q) {
  RC_TRY(map_range(c, which, first, count, "dqn_policy_map"));
  if (count == 0) return P2PMG_OK;
  if (!policy && !q) return fail(c, P2PMG_E_INVALID, "dqn_policy_map: null outputs");
  if (!c->map_axes) RC_TRY(map_default_grid(c, "dqn_policy_map"));
  // chunks of whole networks, or of one network's states, whose bytes fit the staging bound: the policy
  // bytes first, the Q triples behind them at a 256-byte boundary
  const size_t G = c->map_G, per = (policy ? 1 : 0) + (q ? 12 : 0);
  const size_t budget = (size_t)P2PMG_DQN_MAP_STAGE_BYTES - 256;
  size_t cn = 1, gn = G;
  if (G * per <= budget) cn = std::min((size_t)count, budget / (G * per));
  else gn = (budget / per) & ~(size_t)63;
  const size_t q_off = policy ? (cn * gn + 255) & ~(size_t)255 : 0;
  DevBuf<char> staging;
  HIP_TRY(c, staging.alloc(q_off + (q ? cn * gn * 12 : 0)));
  for (size_t k0 = 0; k0 < (size_t)count; k0 += cn) {
    const size_t kn = std::min(cn, (size_t)count - k0);
    for (size_t g0 = 0; g0 < G; g0 += gn) {
      const size_t gc = std::min(gn, G - g0);
      p2pmg::DqnMapParams p = map_params(c, which, first + (int)k0, (int)kn, g0, gc);
      if (policy) p.policy = reinterpret_cast<uint8_t*>(staging.get());
      if (q) p.q = reinterpret_cast<float*>(staging.get() + q_off);
      HIP_TRY(c, p2pmg::launch_dqn_map(p, c->stream));
      if (policy)
        HIP_TRY(c, hipMemcpyAsync(policy + k0 * G + g0, p.policy, kn * gc, hipMemcpyDeviceToHost, c->stream));
      if (q)
        HIP_TRY(c, hipMemcpyAsync(q + (k0 * G + g0) * 3, p.q, kn * gc * 12, hipMemcpyDeviceToHost, c->stream));
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return P2PMG_OK;
}

int p2pmg_dqn_map_stats(p2pmg_ctx* c, int which, int first, int count, double* stats) {
  RC_TRY(map_range(c, which, first, count, "dqn_map_stats"));
  if (count == 0) return P2PMG_OK;
  if (!stats) return fail(c, P2PMG_E_INVALID, "dqn_map_stats: null output");
  if (!c->map_axes) RC_TRY(map_default_grid(c, "dqn_map_stats"));
  p2pmg::DqnMapParams p = map_params(c, which, first, count, 0, c->map_G);
  RC_TRY(map_scratch(c, p));
  HIP_TRY(c, c->map_out.grow((size_t)count * P2PMG_DQN_MAP_STATS));
  p.stat_out = c->map_out;
  HIP_TRY(c, p2pmg::launch_dqn_map(p, c->stream));
  return download(c, {{stats, c->map_out, (size_t)count * P2PMG_DQN_MAP_STATS * sizeof(double)}});
}

int p2pmg_dqn_policy_mark(p2pmg_ctx* c, int which) {
  RC_TRY(map_range(c, which, 0, 0, "dqn_policy_mark"));
  if (!c->map_axes) RC_TRY(map_default_grid(c, "dqn_policy_mark"));
  const bool fresh = !c->map_snap;
  if (fresh && c->map_snap.alloc((size_t)c->n_nets * c->map_G) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, P2PMG_E_NOMEM, "dqn_policy_mark: the map snapshot ([n_nets][G] bytes)");
  }
  p2pmg::DqnMapParams p = map_params(c, which, 0, c->n_nets, 0, c->map_G);
  p.policy = c->map_snap;
  hipError_t e = p2pmg::launch_dqn_map(p, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    if (fresh) c->map_snap.release();  // no half-written first snapshot
    return fail(c, P2PMG_E_HIP, std::string("dqn_policy_mark: ") + hipGetErrorString(e));
  }
  return P2PMG_OK;
}

int p2pmg_dqn_policy_changes(p2pmg_ctx* c, int which, int first, int count, int64_t* changed, int remark) {
  RC_TRY(map_range(c, which, first, count, "dqn_policy_changes"));
  if (!c->map_snap) return fail(c, P2PMG_E_STATE, "dqn_policy_changes: p2pmg_dqn_policy_mark first (a grid change drops the snapshot)");
  if (count == 0) return P2PMG_OK;
  if (!changed) return fail(c, P2PMG_E_INVALID, "dqn_policy_changes: null output");
  p2pmg::DqnMapParams p = map_params(c, which, first, count, 0, c->map_G);
  RC_TRY(map_scratch(c, p));
  HIP_TRY(c, c->map_cout.grow((size_t)count));
  p.snap = c->map_snap.get() + (size_t)first * c->map_G;
  p.remark = remark ? 1 : 0;
  p.chg_out = c->map_cout;
  HIP_TRY(c, p2pmg::launch_dqn_map(p, c->stream));
  std::vector<long long> host((size_t)count);
  RC_TRY(download(c, {{host.data(), c->map_cout, host.size() * sizeof(long long)}}));
  for (int k = 0; k < count; ++k) changed[k] = host[(size_t)k];
  return P2PMG_OK;
}

}  // extern "C"
