// p2pmg_rt_probe.cpp — the probe calls of the parity tests: single device functions (the RC step, the
// divisions, the state index, the battery rule) run over caller arrays through a staging buffer.  Each
// stops at the first HIP error and reports it under its own name.
#include <cmath>

#include "p2pmg_ctx.h"

using namespace p2pmg::rt;

namespace {

p2pmg::RcParams rc_params(const p2pmg_config& g, float solar_gain) {
  return p2pmg::RcParams{g.inv_ci, g.inv_cm, g.inv_ri, g.inv_re, g.inv_rvent, g.one_minus_frad,
                         g.frad, solar_gain, g.hp_cop, g.seconds_per_minute, g.time_slot};
}

// both RC probes stage t_out | t_in | t_m | hp | t_in_new | t_m_new in d[0 .. 6n): the inputs up ...
hipError_t rc_inputs(p2pmg_ctx* c, float* d, size_t n, const float* t_out, const float* t_in, const float* t_m,
                     const float* hp) {
  const float* src[4] = {t_out, t_in, t_m, hp};
  hipError_t e = hipSuccess;
  for (size_t k = 0; k < 4 && e == hipSuccess; ++k) e = hipMemcpyAsync(d + k * n, src[k], n * 4, hipMemcpyHostToDevice, c->stream);
  return e;
}

// ... and, where every step so far succeeded (e), the outputs down
int rc_outputs(p2pmg_ctx* c, hipError_t e, const float* d, size_t n, float* t_in_new, float* t_m_new, const char* what) {
  if (e == hipSuccess) e = hipMemcpyAsync(t_in_new, d + 4 * n, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t_m_new, d + 5 * n, n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return P2PMG_OK;
}

template <typename T, typename L>
int div_check(p2pmg_ctx* c, int n, const T* a, const T* b, T* out, int per, L launch, const char* what) {
  if (!c || n < 0 || (n > 0 && (!a || !b || !out))) return P2PMG_E_INVALID;
  if (n == 0) return P2PMG_OK;
  DevBuf<T> da, db, dout;
  hipError_t e = da.alloc((size_t)n);
  if (e == hipSuccess) e = db.alloc((size_t)n);
  if (e == hipSuccess) e = dout.alloc((size_t)n * per);
  if (e == hipSuccess) e = hipMemcpyAsync(da, a, (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(db, b, (size_t)n * sizeof(T), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch(n, da, db, dout, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * per * sizeof(T), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
  return P2PMG_OK;
}

}  // namespace

extern "C" {

int p2pmg_rc_step(p2pmg_ctx* c, int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                  float* t_in_new, float* t_m_new) {
  if (!c || n < 0 || !t_out || !t_in || !t_m || !hp || !t_in_new || !t_m_new) return P2PMG_E_INVALID;
  if (n == 0) return P2PMG_OK;
  DevBuf<float> d;
  HIP_TRY(c, d.alloc((size_t)6 * n));
  const size_t sn = (size_t)n;
  hipError_t e = rc_inputs(c, d, sn, t_out, t_in, t_m, hp);
  if (e == hipSuccess)
    e = p2pmg::launch_rc_step(n, d, d + sn, d + 2 * sn, d + 3 * sn, d + 4 * sn, d + 5 * sn,
                              rc_params(c->cfg, c->cfg.solar_gain), c->stream);
  return rc_outputs(c, e, d, sn, t_in_new, t_m_new, "rc_step");
}

int p2pmg_rc_step_ex(p2pmg_ctx* c, int n, const float* t_out, const float* t_in, const float* t_m, const float* hp,
                     const float* cop, float solar_gain, float* t_in_new, float* t_m_new) {
  if (!c || n < 0 || !t_out || !t_in || !t_m || !hp || !t_in_new || !t_m_new) return P2PMG_E_INVALID;
  if (n == 0) return P2PMG_OK;
  DevBuf<float> d;
  HIP_TRY(c, d.alloc((size_t)7 * n));  // ... and the per-agent COPs behind them
  const size_t sn = (size_t)n;
  hipError_t e = rc_inputs(c, d, sn, t_out, t_in, t_m, hp);
  if (e == hipSuccess && cop) e = hipMemcpyAsync(d + 6 * sn, cop, sn * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = p2pmg::launch_rc_step_ex(n, d, d + sn, d + 2 * sn, d + 3 * sn, cop ? d + 6 * sn : nullptr, d + 4 * sn,
                                 d + 5 * sn, rc_params(c->cfg, solar_gain), c->stream);
  return rc_outputs(c, e, d, sn, t_in_new, t_m_new, "rc_step_ex");
}

int p2pmg_fdiv_check(p2pmg_ctx* c, int n, const float* a, const float* b, float* out) {
  return div_check(c, n, a, b, out, 4, p2pmg::launch_fdiv_check, "fdiv_check");
}

int p2pmg_fdiv64_check(p2pmg_ctx* c, int n, const double* a, const double* b, double* out) {
  return div_check(c, n, a, b, out, 3, p2pmg::launch_fdiv64_check, "fdiv64_check");
}

int p2pmg_state_indices(p2pmg_ctx* c, int n, const float* obs, int32_t* idx) {
  if (!c || n < 0 || !obs || !idx) return P2PMG_E_INVALID;
  if (n == 0) return P2PMG_OK;
  DevBuf<float> d;
  DevBuf<int32_t> di;
  HIP_TRY(c, d.alloc((size_t)4 * n));
  hipError_t e = di.alloc((size_t)4 * n);
  if (e == hipSuccess) e = hipMemcpyAsync(d, obs, (size_t)16 * n, hipMemcpyHostToDevice, c->stream);
  const p2pmg_config& g = c->cfg;
  if (e == hipSuccess)
    e = p2pmg::launch_state_indices(n, d, di, g.n_time_states, g.n_temp_states, g.n_balance_states, g.n_p2p_states,
                                    c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(idx, di, (size_t)16 * n, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("state_indices: ") + hipGetErrorString(e));
  return P2PMG_OK;
}

int p2pmg_battery_seq(p2pmg_ctx* c, int agents, int steps, const double* bal, double* out_bal, double* soc_hist,
                      double* soc, const double* cap, double smin, double smax, double eff) {
  if (!c || agents < 0 || steps < 0 || !bal || !out_bal || !soc_hist || !soc || !cap) return P2PMG_E_INVALID;
  const size_t n = (size_t)agents * steps;
  DevBuf<double> d;
  HIP_TRY(c, d.alloc(3 * n + 2 * (size_t)agents + 1));
  double *db = d, *dob = d + n, *dsh = d + 2 * n, *ds = d + 3 * n, *dc = d + 3 * n + agents;
  hipError_t e = hipMemcpyAsync(db, bal, n * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ds, soc, (size_t)agents * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dc, cap, (size_t)agents * 8, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = p2pmg::launch_battery_seq(agents, steps, db, dob, dsh, ds, dc, smin, smax, std::sqrt(eff), c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(out_bal, dob, n * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(soc_hist, dsh, n * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(soc, ds, (size_t)agents * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(c, P2PMG_E_HIP, std::string("battery_seq: ") + hipGetErrorString(e));
  return P2PMG_OK;
}

}  // extern "C"
