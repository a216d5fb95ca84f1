// p2pmg_fastmath.h — what the fast paths (p2pmg_fast.hip, p2pmg_sq16.hip, and p2pmg_small.hip's pre-pass,
// record-unpack, rule and fdiv*_check kernels) share beyond p2pmg_tabular.h: the range-free f32 / f64 quotients
// and the battery rule on them, the T0 draw, the step pre-pass and the packed record row.
#pragma once
#include "p2pmg_tabular.h"

namespace p2pmg {
namespace {

// IEEE f32 division a / b without its range handling.  hipcc's correctly rounded sequence is
//   v_div_scale(b), v_rcp, y = fma(fma(-b, rcp, 1), rcp, rcp), v_div_scale(a),
//   q = a*y, r = fma(-b, q, a), q = fma(r, y, q), r = fma(-b, q, a), v_div_fmas = fma(r, y, q),
//   v_div_fixup
// The two scale steps are identities (and v_div_fmas a plain fma) while |a| and |b| lie in
// [2^-40, 2^40] (exponent gap below 96, nothing near denormal or overflow), and v_div_fixup only
// rewrites NaN / inf / zero / denormal cases, none of which a quotient of two such numbers is.
// So inside that range these five ops ARE the division, bit for bit; outside it, or for a = 0,
// the caller takes the IEEE operator.  The reciprocal of a loop-invariant divisor (max_in, the
// 60 minutes of an hour, N, the comfort margin) is hoisted out of the episode loop.
struct Recip {
  float b, y;
  bool ok;  // |b| in range
};
__device__ __forceinline__ bool in_div_range(float x) {
  const float m = fabsf(x);
  return m >= 0x1p-40f && m <= 0x1p40f;
}
__device__ __forceinline__ Recip recip(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  return Recip{b, __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0), in_div_range(b)};
}
// ONE Newton correction of q0 = a y suffices (round 5): with y refined from v_rcp_f32 as in recip(),
// q = fma(fma(-b, q0, a), y, q0) equals the IEEE quotient for every pair of 24-bit significands
// (all 2^46 pairs checked on the GPU, scripts/div_exhaustive.hip, profiles/r05_div_exhaustive.jsonl),
// v_rcp_f32 scales exactly with the divisor's exponent (same run, e in [-40, 40]), and inside the
// range every step scales exactly with the operands' exponents (the residual stays representable),
// so the significand pairs decide every case.  The second correction of rounds 1-4 was a no-op.
__device__ __forceinline__ float fdiv_core(float a, const Recip& d) {
  const float q0 = a * d.y;
  const float r = __builtin_fmaf(-d.b, q0, a);
  const float q = __builtin_fmaf(r, d.y, q0);
  // a = +-0: the steps above give +0; the IEEE quotient carries sign(a) * sign(b) = sign(q0).
  // For every other a the sign of q already equals sign(q0), so the copy is exact either way.
  return __builtin_copysignf(q, q0);
}
__device__ __forceinline__ bool fdiv_ok(float a) {
  const float m = fabsf(a);
  return (m >= 0x1p-40f && m <= 0x1p40f) || m == 0.0f;
}
// the IEEE quotient behind an opaque copy of a: keeps the compiler from speculating this rare path
// (11 instructions) into a select on the common one
__device__ __forceinline__ float fdiv_ieee(float a, float b) {
  asm volatile("" : "+v"(a));
  return a / b;
}
// a / b with a divisor the launcher has checked to lie in range (max_in, 60, N, the margin)
__device__ __forceinline__ float fdiv_b(float a, const Recip& d) {
  float q = fdiv_core(a, d);
  if (!fdiv_ok(a)) q = fdiv_ieee(a, d.b);  // rare: tiny, huge or non-finite numerator
  return q;
}
template <int N>
__device__ __forceinline__ float div_n_r(float x, const Recip& rn) {
  if constexpr ((N & (N - 1)) == 0) return x * (1.0f / (float)N);
  else return fdiv_b(x, rn);
}
// clamp_bin as one v_med3: (int)med3(v, 0, K-1) equals clamp_bin for every non-NaN v (values in
// [0, 1) truncate to 0 like the reference's v < 1 branch)
__device__ __forceinline__ int clamp_bin_f(float v, float km1) { return (int)__builtin_amdgcn_fmed3f(v, 0.0f, km1); }

// T0 ~ N(setpoint, sigma) for (episode, global agent id): Box-Muller on one Philox block
// (HPHeating.reset heating.py:145-152 with a counter-based stream; oracle/philox.py t0_draws)
__device__ __forceinline__ void t0_draw(uint32_t k0, uint32_t k1, int episode, uint32_t gid, float setpoint,
                                        double sigma, float& t_in, float& t_m) {
  uint32_t c0 = 0, c1 = (uint32_t)episode, c2 = gid, c3 = kTagT0;
  philox4x32_10(c0, c1, c2, c3, k0, k1);
  const double u1 = ((double)c0 + 0.5) / 4294967296.0;
  const double u2 = ((double)c1 + 0.5) / 4294967296.0;
  const double rad = sqrt(-2.0 * log(u1));
  const double ang = 6.283185307179586 * u2;
  t_in = (float)((double)setpoint + sigma * (rad * cos(ang)));
  t_m = (float)((double)setpoint + sigma * (rad * sin(ang)));
}
// Step pre-pass: everything of step t that depends only on the inputs (profiles, environment,
// max_in), not on the policy or the temperatures, for every (t, agent) in one parallel launch per
// episode, so the serial episode loop pays for none of these divisions and bins:
//   pre[t][a].x = bits of balw = ((load - pv) / max_in) * max_in      agent.py:172-176, 210
//   pre[t][a].y = (it_t * nT*nb + ib_t) | (it_{t+1} * nT*nb + ib_{t+1}) << 16
//                 (row / np of the state (it, 0, ib, 0) and of the next state, rl.py:89-95;
//                  the next state's balance is that of the next profile row, wrapping at T)
// PHILOX = true also writes the step's exploration code words (philox_codes_kernel's job).
// ep: the episode of a chain (o.n_ep > 1) whose code words to write; the policy-independent words
// are the same for every episode and written with episode 0's.
__device__ __forceinline__ void prepass_one(const EpisodeParams& p, const PrepOut& o, size_t k, int ep = 0) {
  const int t = (int)(k / p.A), a = (int)(k % p.A);
  const int tn = t + 1 == p.T ? 0 : t + 1;
  const int se = p.n_env == 1 ? 0 : a / p.N;
  const float mi = p.max_in[a];
  const float2 f = p.prof[k], fn = p.prof[(size_t)tn * p.A + a];
  const float bal = (f.x - f.y) / mi, baln = (fn.x - fn.y) / mi;
  const float time_t = p.env[((size_t)t * p.n_env + se) * kEnvStride];
  const float time_n = p.env[((size_t)tn * p.n_env + se) * kEnvStride];
  const uint32_t tb = (uint32_t)(p.nT * p.nb);
  const uint32_t lo = (uint32_t)idx_time(time_t, p.nt) * tb + (uint32_t)idx_plain(bal, p.nb);
  const uint32_t hi = (uint32_t)idx_time(time_n, p.nt) * tb + (uint32_t)idx_plain(baln, p.nb);
  if (ep == 0) o.pre[k] = make_uint2(__float_as_uint(bal * mi), lo | (hi << 16));
  if (o.ipc && ep == 0) {
    // N = 2: round 1's p2p feature depends only on the partner's round-0 action b (agent.py:203):
    // its column entry is ev_b = ((balw_p + hp_p[b]) * 1) / 2 (the even split of round 0), summed
    // as in the kernel's acc loop.  Byte b = the bin for b, so the kernel's round-1 rows can be
    // issued a step ahead and picked by the partner's action.
    const int i = a % 2, ap = a ^ 1;
    const float2 fp = p.prof[(size_t)t * p.A + ap];
    const float mip = p.max_in[ap];
    const float balw_p = ((fp.x - fp.y) / mip) * mip;
    const float4 lvp = p.hp_lv[ap];
    const float hpl[3] = {lvp.x, lvp.y, lvp.z};
    uint32_t ipc = 0;
    for (int b = 0; b < 3; ++b) {
      const float ev = div_n<2>((balw_p + hpl[b]) * 1.0f);
      float acc = 0.0f;
      for (int j = 0; j < 2; ++j) acc = acc + (-((j == i) ? 0.0f : ev));
      ipc |= (uint32_t)idx_plain(div_n<2>(acc) / mi, p.np) << (8 * b);
    }
    o.ipc[k] = ipc;
  }
  if (o.words) {
    EpisodeParams q = p;
    const bool chain = o.n_ep > 1;
    q.episode = o.episode + ep;
    q.eps = o.eps;
    q.eps_thr = chain ? o.ep_thr[ep] : o.eps_thr;
    q.eps_all = chain ? (int)((o.ep_all >> ep) & 1u) : o.eps_all;
    if (o.eps_tab) {  // the scenario's own threshold of this episode (p2pmg_run_episodes_eps)
      const uint2 e = o.eps_tab[(size_t)ep * p.S + a / p.N];
      q.eps_thr = e.x;
      q.eps_all = (int)e.y;
    }
    const int R1 = p.R + 1, W = (R1 + 3) >> 2;
    const uint32_t gid = p.agent_offset + (uint32_t)a;
    const uint64_t codes = philox_codes_of(q, t, gid);
    uint32_t* words = o.words + (size_t)ep * o.words_stride;
    for (int w = 0; w < W; ++w)
      words[((size_t)t * W + w) * p.A + a] =
          w < 2 ? (uint32_t)(codes >> (32 * w))
                : philox_code_word(t, R1, w, (uint32_t)q.episode, gid, q.eps_thr, q.eps_all, p.seed_lo, p.seed_hi);
  }
}

// f64 division with a hoisted reciprocal: hipcc's IEEE f64 sequence (v_div_scale, v_rcp_f64, two
// Newton steps, q = n * y, r = fma(-d, q, n), v_div_fmas = fma(r, y, q), v_div_fixup) with the
// scale / fixup steps dropped, which is exact while |n| and |d| lie in [2^-300, 2^300] (the
// exponent gap stays below the 768 where v_div_scale starts scaling); else the IEEE operator.
struct Recip64 {
  double d, y;
  bool ok;
};
__device__ __forceinline__ bool in_div_range64(double x) {
  const double m = fabs(x);
  return m >= 0x1p-300 && m <= 0x1p300;
}
__device__ __forceinline__ Recip64 recip64(double d) {
  const double r0 = __builtin_amdgcn_rcp(d);
  const double r1 = __builtin_fma(r0, __builtin_fma(-d, r0, 1.0), r0);
  return Recip64{d, __builtin_fma(r1, __builtin_fma(-d, r1, 1.0), r1), in_div_range64(d)};
}
// x / 900 s (storage.py) through the correctly rounded reciprocal as a compile-time constant: the
// one Newton correction in qcore64 / qpos64 returns the IEEE quotient from it as from the device's
// refined v_rcp_f64 estimate, and a literal is rematerialised where a kernel-argument-derived value
// would hold two SGPRs across the loop (or spill them to VGPR lanes)
constexpr Recip64 kR900{900.0, 1.0 / 900.0, true};
__device__ __forceinline__ double fdiv64_ieee(double n, double d) {
  asm volatile("" : "+v"(n));
  return n / d;
}
__device__ __forceinline__ double fdiv64(double n, const Recip64& r) {
  const double q = n * r.y;
  double res = __builtin_fma(__builtin_fma(-r.d, q, n), r.y, q);
  res = __builtin_copysign(res, q);  // +-0 / d keeps sign(n) * sign(d), as the IEEE quotient
  if (!(r.ok && (n == 0.0 || in_div_range64(n)))) res = fdiv64_ieee(n, r.d);
  return res;
}
// reciprocals of kernel-uniform divisors, moved to SGPRs (v_readfirstlane): VGPRs set the
// occupancy of the throughput-bound sq16 kernel
__device__ __forceinline__ float sgpr_f(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ double sgpr_d(double x) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
__device__ __forceinline__ Recip recip_u(float b) {
  const Recip r = recip(b);
  return Recip{b, sgpr_f(r.y), r.ok};
}
__device__ __forceinline__ Recip64 recip64_u(double d) {
  const Recip64 r = recip64(d);
  return Recip64{d, sgpr_d(r.y), r.ok};
}
// battery_rule (agent.py:138-153 + storage.py bookkeeping) with the divisions by the agent's
// capacity, sqrt(efficiency) and 900 s through hoisted reciprocals; same op order, same results.
// Branch-free: the discharge and charge branches divide the same expressions of their own x, so x
// is selected first and x / cap, x / 900, (x / cap) / sqrt(eff) are computed once (4 quotients
// instead of up to 6 on a divergent wave); one range test for all of them, and a lane with an
// operand outside the range-free quotient's domain redoes the rule with IEEE divisions.
struct BatK {
  double smin, smax, se;
  Recip64 rse, r900;
};
// 0, or |n| in [2^-300, 2^300) by its biased exponent (723..1322): the range-free quotient's domain
__device__ __forceinline__ bool q64_ok(double n) {
  const unsigned e = ((unsigned)__double2hiint(n) >> 20) & 0x7FFu;
  return (e - 723u <= 599u) || n == 0.0;
}
// fdiv64 without its range test (the caller tests the operands)
__device__ __forceinline__ double qcore64(double n, const Recip64& r) {
  const double q = n * r.y;
  return __builtin_copysign(__builtin_fma(__builtin_fma(-r.d, q, n), r.y, q), q);
}
// CHECK = false: the launcher has verified the operands' domain (p2pmg_set_battery / set_profiles:
// capacities 0 or in [2^-20, 2^60], SoC bounds in [2^-100, 2^10], sqrt(eff) in [2^-10, 2^10], SoC0 in
// [0, 2^10], |load|, |pv|, heat-pump levels <= 2^100).  Then every numerator is 0 or in
// [2^-252, 2^168] (a positive SoC - bound difference is a multiple of the bound's ulp >= 2^-152; a
// nonzero f32 balance times 900 lies in [2^-140, 2^138]) and the per-lane range tests go.
// The SoC-only terms of the rule (storage.py:52-60: available energy / space, the full test), the
// same for every round of a step: computed once per step (bat_pre) and shared by the rounds.
struct BatPre {
  double avail_energy, avail_space;
  bool full;
};
// x / d for d > 0 and x >= +0: qcore64 without the sign fix, which only matters for x = -0
__device__ __forceinline__ double qpos64(double n, const Recip64& r) {
  const double q = n * r.y;
  return __builtin_fma(__builtin_fma(-r.d, q, n), r.y, q);
}
__device__ __forceinline__ BatPre bat_pre(double soc, double cap, const BatK& b) {
  // space >= +0 (fmax with 0, a positive capacity), so the unsigned quotient is the IEEE one
  return BatPre{(fmax(0.0, soc - b.smin) * cap) * b.se, qpos64(fmax(0.0, b.smax - soc) * cap, b.rse), soc >= b.smax};
}
// battery_rule_r<false> on a step's precomputed SoC terms (the launcher-verified domain): every
// quotient's numerator is positive where it is used (dis: x = min(energy, avail_energy) > 0;
// chg: x = min(-energy, avail_space) > 0 as soc < smax), so the quotients need no sign fix
// (balance * 60) * 15 of a balance that is an f32 value: both products are exact in f64 (24 + 4 + 4
// significant bits), and so is balance * 900 (24 + 8): one multiply, the same double
__device__ __forceinline__ double energy_of(double balance_f32) { return balance_f32 * 900.0; }
// -x if c else x: a sign flip of the high word (x - y == x + (-y) in IEEE arithmetic)
__device__ __forceinline__ double neg_if(double x, bool c) {
  return __hiloint2double(__double2hiint(x) ^ (c ? (int)0x80000000 : 0), __double2loint(x));
}
__device__ __forceinline__ double battery_rule_pre(double balance, double& soc, const Recip64& rcap, const BatK& b,
                                                   const BatPre& pr) {
  const double energy = energy_of(balance);
  const bool dis = balance > 0.0 && pr.avail_energy > 0.0;
  const bool chg = !dis && balance < 0.0 && !pr.full;
  // min(energy, available_energy) / min(-energy, available_space) as v_min_f64 (IEEE minNum): in the
  // launcher-verified domain every operand is finite, and where x is used both are positive (dis:
  // energy > 0, avail_energy > 0; chg: -energy > 0, avail_space >= +0), so minNum returns what the
  // reference's `a <= b ? a : b` does (equal values are the same double); 4 VALU instead of 9
  const double x = dis ? fmin(energy, pr.avail_energy) : fmin(-energy, pr.avail_space);
  const double q1 = qpos64(x, rcap);     // x / capacity
  const double q2 = qpos64(x, b.r900);   // x / 900
  const double q3 = qpos64(q1, b.rse);   // (x / capacity) / sqrt(eff)
  // dis: soc - q3, balance - q2; chg: soc + sqrt(eff) q1, balance + q2 -- one add each
  const double soc_n = soc + (dis ? neg_if(q3, true) : b.se * q1);
  const double bal_n = balance + neg_if(q2, dis);
  soc = (dis || chg) ? soc_n : soc;
  return (dis || chg) ? bal_n : balance;
}
template <bool CHECK = true>
__device__ __forceinline__ double battery_rule_r(double balance, double& soc, double cap, const Recip64& rcap,
                                                 const BatK& b) {
  const double energy = energy_of(balance);  // (balance * 60) * 15, exact for the f32 balances passed in
  const double avail_energy = (fmax(0.0, soc - b.smin) * cap) * b.se;
  const double space_n = fmax(0.0, b.smax - soc) * cap;
  const double avail_space = qcore64(space_n, b.rse);
  const bool dis = balance > 0.0 && avail_energy > 0.0;
  const bool chg = !dis && balance < 0.0 && !(soc >= b.smax);
  const double x = dis ? (energy <= avail_energy ? energy : avail_energy)    // min(energy, available_energy)
                       : (-energy <= avail_space ? -energy : avail_space);  // min(-energy, available_space)
  const double q1 = qcore64(x, rcap);     // x / capacity
  const double q2 = qcore64(x, b.r900);   // x / 900
  const double q3 = qcore64(q1, b.rse);   // (x / capacity) / sqrt(eff)
  if constexpr (CHECK) {
    const bool ok = rcap.ok && b.rse.ok && b.r900.ok && q64_ok(x) && q64_ok(q1) && (!chg || q64_ok(space_n));
    if ((dis || chg) && !ok) return battery_rule(balance, soc, cap, b.smin, b.smax, b.se);  // IEEE divisions
  }
  const double soc_n = dis ? soc - q3 : soc + b.se * q1;
  const double bal_n = dis ? balance - q2 : balance + q2;
  soc = (dis || chg) ? soc_n : soc;
  return (dis || chg) ? bal_n : balance;
}

// the sq16 kernel's packed quotient (here for fdiv_check_kernel, which runs every guarded form)
typedef float pkf2 __attribute__((ext_vector_type(2)));
// 0 or |x| in [2^-19, 2^19]: products of two such numbers are 0 or in [2^-38, 2^38]
__device__ __forceinline__ bool in_range19(float x) {
  const float m = fabsf(x);
  return m == 0.0f || (m >= 0x1p-19f && m <= 0x1p19f);
}
// fdiv_core on a packed pair with the residual negated, r' = b q0 - a: the same quotient bit for
// bit (round-to-nearest is sign-symmetric, and an exact-zero residual is +0 either way, which
// leaves q unchanged), and for a = +-0 with a POSITIVE divisor (the only use: tot = |sum| > 0) it
// keeps sign(a) without fdiv_core's copysign: q0 = +-0, r' = +0, q = fma(-0, y, +-0) = +-0.  (With
// a negative divisor q0 = -+0 and the last fma returns +0 for a = +0: not the IEEE -0; the division
// fuzz test checks the positive-divisor domain.)  Both lanes round like the scalar fma.
__device__ __forceinline__ pkf2 fdiv_core_pk(pkf2 a, pkf2 b, pkf2 y) {
  // q0 as two scalar multiplies: v_mul_f32 issues at 2.6 SIMD cycles, v_pk_mul_f32 at 6.6
  // (profiles/r04_ubench_rate.jsonl); the FMAs stay packed (v_pk_fma_f32 6.8 < 2 x 3.8)
  const pkf2 q0 = {a.x * y.x, a.y * y.y};
  const pkf2 r = __builtin_elementwise_fma(b, q0, -a);
  return __builtin_elementwise_fma(-r, y, q0);  // one correction, as fdiv_core
}

// One packed record row of episode_fast_kernel / episode_sq16_kernel (fast_rec_unpack_kernel, p2pmg_summary.hip)
struct FastRec {         // [T][A], 32 B
  float reward, cost, grid, p2p, tin;
  uint32_t actions;      // byte r: action of round r
  uint32_t bins;         // (it * nT*nb + ib) | iT << 16
  uint32_t ips;          // byte r: p2p bin of round r
};

}  // namespace
}  // namespace p2pmg
