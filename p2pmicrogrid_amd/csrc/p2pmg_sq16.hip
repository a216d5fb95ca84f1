// p2pmg_sq16.hip — episode_sq16_kernel, the throughput-bound shared-table path for 16-agent scenarios,
// and its per-upload pre-pass.  _build.py compiles this unit with -fno-slp-vectorize.
#include "p2pmg_fastmath.h"

namespace p2pmg {
namespace {

// ----------------------------------------------------------------- the fast shared-table path (N = 16)
// __double2ll_rn(x) in two VALU ops while |x| < 2^51: y = x + 1.5 * 2^52 lies in [2^52, 2^53), where
// the f64 spacing is 1, so the add IS the round-to-nearest-even, and the integer sits in y's
// significand: int64 = bits(y) - bits(1.5 * 2^52), whose low word is 0 (only the high word changes,
// no borrow).  Otherwise (a TD delta of 2^11 or more, wave-uniformly tested) the library conversion.
__device__ __forceinline__ long long rne_ll(double x) {
  if (__all(fabs(x) < 0x1p51)) {
    const double y = x + 0x1.8p52;
    const unsigned lo = (unsigned)__double2loint(y);
    const unsigned hi = (unsigned)__double2hiint(y) - 0x43380000u;
    return (long long)(((unsigned long long)hi << 32) | lo);
  }
  return __double2ll_rn(x);
}

// v with lane (16 k + J) set to +0 for every k: the diagonal of a 16-agent scenario whose agent i
// sits in lane i of its 16-lane group.  The lane pattern is a constant loaded into VCC right at the
// use: as a C++ compare, the 16 loop-invariant masks get hoisted into 32 SGPRs, spill to VGPR lanes
// and cost two v_readlane per use.
template <int J>
__device__ __forceinline__ float zero_diag16(float v) {
  float r;
  asm volatile("s_mov_b32 vcc_lo, %2\n\ts_mov_b32 vcc_hi, %2\n\tv_cndmask_b32_e64 %0, %1, 0, vcc"
               : "=v"(r) : "v"(v), "i"(0x00010001u << J) : "vcc");
  return r;
}
template <int J = 0>
__device__ __forceinline__ void zero_diag16_all(float (&col)[16]) {
  if constexpr (J < 16) {
    col[J] = zero_diag16<J>(col[J]);
    zero_diag16_all<J + 1>(col);
  }
}
// episode_sq16_kernel: episode_kernel's shared-table path for 16-agent scenarios (configs[2]),
// rebuilt for throughput: 1M scenarios keep every SIMD busy, so the cost is instructions per
// agent-step, not latency.  Same op order and results as episode_kernel (tests compare both).
//   * round 0 is an even split: round 1's column is the 16 round-0 values of the group, one LDS
//     write + four 16-B reads instead of a 16 x 16 exchange;
//   * the divisions of _divide_power share one divisor per round (hoisted reciprocal), the
//     battery's f64 divisions share the agent's capacity / sqrt(eff) / 900 s reciprocals;
//   * the final 16 x 16 proposal matrix is transposed through a swizzled LDS tile (4 x 16-B
//     writes, 16 conflict-free 4-B reads);
//   * the table is frozen for the episode: TD deltas go to the workgroup's LDS hash as before.
#ifndef P2PMG_SQ16_OCC
#define P2PMG_SQ16_OCC 4  // min waves per SIMD the register allocation must allow (LDS allows 4)
#endif
constexpr int kSq16Waves = 8;                        // waves per workgroup (one hash per 32 scenarios)
constexpr int kTpStride = 16 * 16 + 16;              // floats per scenario tile (+16: bank offset)
// BAT: 0 none, 1 battery with per-lane range tests, 2 battery in the launcher-verified domain
template <typename QT, int R1, bool TRAIN, int BAT, bool NARROW>
__global__ __launch_bounds__(kWave * kSq16Waves, P2PMG_SQ16_OCC) void episode_sq16_kernel(const EpisodeParams p) {
  constexpr int N = 16, G = 16, SPW = kWave / G;
  __shared__ uint32_t hkey[kSqSlots];
  __shared__ unsigned long long hval[kSqSlots];
  __shared__ double tdk[2];  // {alpha, gamma} of the TD update, read per step (see below)
  __shared__ __attribute__((aligned(16))) float tpall[kSq16Waves * SPW * kTpStride];
  const int wv = (int)(threadIdx.x / kWave);
  const int lane = (int)(threadIdx.x % kWave);
  const int sl = lane / G;
  const int i = lane % G;
  const int s = (blockIdx.x * kSq16Waves + wv) * SPW + sl;
  const bool active = s < p.S;
  const int a = active ? s * N + i : 0;
  const int s_env = p.n_env == 1 ? 0 : (active ? s : 0);
  const int T = p.T;
  const size_t A = (size_t)p.A;
  const KC k = scalar_constants(p);
  const Dims<true> D{k.nt, k.nT, k.nb, k.np};
  // the launcher sends this kernel 20^4 tables only (p2pmg_plan.cpp, the Sq16 family): the state
  // count is a literal, not four kernel arguments kept in SGPRs across the loop
  constexpr uint32_t n_states = 20u * 20u * 20u * 20u;
  const QT* __restrict__ q = reinterpret_cast<const QT*>(p.q);
  unsigned long long* const dbase = reinterpret_cast<unsigned long long*>(p.qdelta) +
                                    (size_t)(blockIdx.x % kDeltaCopies) * n_states * kQPad;
  for (int k2 = threadIdx.x; k2 < kSqSlots; k2 += kSq16Waves * kWave) {
    hkey[k2] = kSqEmpty;
    hval[k2] = 0;
  }
  if (threadIdx.x == 0) {
    tdk[0] = p.alpha;
    tdk[1] = p.gamma;
  }
  __syncthreads();
  float* const tp = tpall + (wv * SPW + sl) * kTpStride;  // this scenario's tile
  // column reads of the transpose: element i of row j sits at j*16 + 4*((i>>2) ^ (j&3)) + (i&3)
  int cofs[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) cofs[m] = 4 * ((i >> 2) ^ m) + (i & 3);

  const float mi = active ? p.max_in[a] : 1.0f;
  const Recip rmi = recip(mi), rmph = recip_u(k.mph), rmargin = recip_u(k.margin);
  const float4 lv = p.hp_lv[a];
  // margin == 1 (the reference's) tested per step as a scalar compare of its bits: a loop-invariant
  // bool would be kept as a 64-bit lane mask across the loop (two SGPRs, spilled to VGPR lanes)
  const uint32_t margin_bits = __float_as_uint(p.margin);
  auto margin_one = [&]() __attribute__((always_inline)) {
    uint32_t r;
    asm volatile("s_cmp_eq_u32 %1, 0x3f800000\n\ts_cselect_b32 %0, 1, 0" : "=s"(r) : "s"(margin_bits) : "scc");
    return r != 0;
  };
  double bcap = 0.0, soc = 0.0;
  BatK bk{};
  Recip64 rcap{};
  if constexpr (BAT != 0) {
    bcap = p.bat_cap[a];
    soc = p.soc[a];
    bk = BatK{p.bat_min, p.bat_max, p.bat_sqrt_eff, recip64_u(p.bat_sqrt_eff), kR900};
    rcap = recip64(bcap > 0.0 ? bcap : 1.0);
  }
  float tin = active ? p.t_in[a] : k.setpoint;
  float tm = active ? p.t_m[a] : k.setpoint;
  const int ip_zero = idx_plain(div_n<N>(0.0f) / mi, D.p());
  const int R1r = p.R + 1, W = (R1r + 3) >> 2;

  // running element offsets in 32 bits (the launcher checks T * A * W < 2^32 and the env table
  // size): fewer 64-bit uniform values live across the loop, i.e. fewer SGPR spills
  // (one wrapped step index, t + 2 mod T, and the offsets as scalar products of it: fewer uniform
  // values live across the loop than three running offsets and their wrap points)
  const float* envb = p.env + (size_t)s_env * kEnvStride;
  const uint32_t env_step = (uint32_t)p.n_env * kEnvStride;
  // the policy-independent per-step words {balance, it * 8000 + ib * 20} (sq16_prep_kernel)
  const uint2* sqpb = p.sqp + a;
  const uint32_t A32 = (uint32_t)p.A;
  const uint32_t* codes_a = p.codes + a;
  const uint32_t code_step = (uint32_t)W * A32;
  const uint32_t T32 = (uint32_t)T;
  const uint32_t t1 = T32 > 1 ? 1u : 0u;
  uint32_t t2 = (2u % T32);  // step t + 2 (mod T) of the loop's iteration t
  const uint32_t f1o = t1 * A32;
  // records: FastRec rows, or only {reward, cost} as float2 when nothing else was requested
  // (8 B instead of 32 B of writes per agent-step); masked-off lanes write a dummy row.  Compile
  // time, as in the fast kernel: no store-count branch for the vmcnt bookkeeping to be pessimistic about
  constexpr bool narrow = NARROW;
  const size_t rec_bytes = narrow ? sizeof(float2) : sizeof(FastRec);
  char* const rec_dummy = reinterpret_cast<char*>(reinterpret_cast<FastRec*>(p.dummy) + kWave + lane);
  const bool rec_on = p.record != 0 && active;
  char* rec_ptr = rec_on ? reinterpret_cast<char*>(p.rec_pack) + (size_t)a * rec_bytes : rec_dummy;
  const size_t rec_step = rec_on ? A * rec_bytes : 0;

  const uint2 w0 = sqpb[0];
  uint2 w1 = sqpb[f1o];
  // step t's state: the balance and the time / balance part of the row offset come precomputed
  // (w: step t, wn: step t + 1 for the next-state row); only the temperature bin depends on the
  // policy: rl.py:89-95 as one v_med3 + convert (clamp_bin_f == clamp_bin for every non-NaN value)
  auto step_idx = [&](uint2 w, uint2 wn, float t_in) {
    StepIdx st;
    st.bal = __uint_as_float(w.x);
    const float dt = t_in - k.setpoint;
    const float tnorm = margin_one() ? dt : fdiv_b(dt, rmargin);
    st.iT = clamp_bin_f(((tnorm + 1.0f) / 2.0f) * 18.0f + 1.0f, 19.0f);
    const uint32_t tT = __umul24((uint32_t)st.iT, 400u);
    st.strip = w.y + tT;
    st.nrow = wn.y + tT + (uint32_t)ip_zero;
    st.it = (int)w.y;  // it * 8000 + ib * 20: the records' bins are w.y / 20 (records only)
    return st;
  };
  // the shared table's rows as 32-bit offsets from its (uniform) base: global_load's SGPR-base +
  // VGPR-offset form instead of a 64-bit address per row (the table spans < 4 GiB)
  const char* const qb = reinterpret_cast<const char*>(q);
  constexpr uint32_t kRowShift = sizeof(QT) == 8 ? 5 : 4;
  auto gatq = [&](uint32_t row) __attribute__((always_inline)) {
    return gather_row(reinterpret_cast<const QT*>(qb + (row << kRowShift)));
  };
  StepIdx st = step_idx(w0, w1, tin);
  // R + 1 = 2 in-kernel Philox: one block holds the codes of two steps (p2pmg_device.h), computed
  // at the even step and kept for the odd one in the code word's unused high half
  constexpr bool kPair = R1 == 2 && TRAIN;
  const bool rng1 = p.rng == 1;
  auto block2 = [&](uint32_t blk) -> uint64_t {
    const uint32_t c4 = philox_block_codes(blk, (uint32_t)p.episode, p.agent_offset + (uint32_t)a, p.eps_thr, p.eps_all,
                                           p.seed_lo, p.seed_hi);
    return (uint64_t)(c4 & 0xFFFFu) | ((uint64_t)(c4 >> 16) << 32) | 0xFFFF0000FFFF0000ull;
  };
  uint64_t cw = code_word_t<TRAIN>(p, step_codes(p, codes_a, 0, 0, a, W, !kPair));
  if (kPair && rng1) cw = block2(0);
  auto row0_addr = [&](const StepIdx& x, uint64_t c) -> uint32_t {
    const bool need = ((c & 0xFF) == 255) || (TRAIN && R1 == 1);
    return need ? x.strip + (uint32_t)ip_zero : x.nrow;
  };
  uint32_t a0 = row0_addr(st, cw);
  Row4<QT> row0 = gatq(a0);
  Row4<QT> rowN = gatq(TRAIN ? st.nrow : a0);
  float ep_sum = 0.0f;

  for (int t = 0; t < T; ++t) {
    const uint32_t t1n = t + 1 == T ? 0u : (uint32_t)t + 1u;  // step t + 1 (mod T)
    // step t's env row {t_out, prices} at the top of the step, not carried across the loop: its first
    // use (the RC update) is half a step of this wave's issue away, which the SIMD's other waves fill
    const EnvRow e0 = load_env(envb + (uint32_t)t * env_step);
    const uint2 w2 = sqpb[t2 * A32];
    const CodeWords cw1r = step_codes(p, codes_a, t1n * code_step, (int)t1n, a, W, !kPair);
    const float balw = st.bal * mi;
    float row[N];
    float col[N];

    // round 0 (P = 0: even split); the battery adjusts the tentative net power
    int code = (int)(cw & 0xFF);
    int act = code == 255 ? argmax3(row0) : code;
    float hp = hp_of(lv, act);
    int ip = ip_zero;
    Row4<QT> rowR = row0;
    uint32_t acts = (uint32_t)act, ips = (uint32_t)ip_zero;
    double soc_r = soc;
    float out = balw + hp;
    BatPre bpre{};
    if constexpr (BAT == 2) bpre = bat_pre(soc, bcap, bk);  // shared by the step's two rounds
    auto bat_rule = [&](float o, double& sr) -> float {
      if constexpr (BAT == 2) return (float)battery_rule_pre((double)o, sr, rcap, bk, bpre);
      return (float)battery_rule_r<true>((double)o, sr, bcap, rcap, bk);
    };
    if constexpr (BAT != 0) {
      if (bcap > 0.0) out = bat_rule(out, soc_r);
    }
    const float ev0 = div_n<N>(out * 1.0f);
    const bool ok_ev0 = in_range19(ev0);
#pragma unroll
    for (int j = 0; j < N; ++j) row[j] = ev0;
    if constexpr (R1 == 2) {
      // round 1: the column is the group's 16 round-0 values
      tp[i] = ev0;
      wave_lds_fence();
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const float4 v = *reinterpret_cast<const float4*>(tp + 4 * m);
        col[4 * m] = v.x; col[4 * m + 1] = v.y; col[4 * m + 2] = v.z; col[4 * m + 3] = v.w;
      }
      wave_lds_fence();
      zero_diag16_all(col);  // powers = -P[:, i] with P's diagonal zeroed (community.py:76,81)
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < N; ++j) acc = acc + (-col[j]);
      ip = clamp_bin_f(((fdiv_b(div_n<N>(acc), rmi) + 1.0f) / 2.0f) * 20.0f, 19.0f);
      code = (int)((cw >> 8) & 0xFF);
      const bool need = code == 255 || TRAIN;
      rowR = gatq(need ? st.strip + (uint32_t)ip : a0);
      act = code == 255 ? argmax3(rowR) : code;
      acts |= (uint32_t)act << 8;
      ips |= (uint32_t)ip << 8;
      hp = hp_of(lv, act);
      out = balw + hp;
      soc_r = soc;
      if constexpr (BAT != 0) {
        if (bcap > 0.0) out = bat_rule(out, soc_r);
      }
      const float flo = out < 0.0f ? 0.0f : -__builtin_inff(), fhi = out > 0.0f ? 0.0f : __builtin_inff();
      float f[N];
      float tot = 0.0f;
#pragma unroll
      for (int j = 0; j < N; ++j) {
        f[j] = __builtin_amdgcn_fmed3f(-col[j], flo, fhi);
        tot = tot + f[j];
      }
      tot = fabsf(tot);
      const float ev = div_n<N>(out * 1.0f);
      const Recip rt = recip(tot == 0.0f ? 1.0f : tot);
      const float nout = nabs_out(out);
      float num[N];
#pragma unroll
      for (int j = 0; j < N; ++j) num[j] = nout * f[j];
      // One wave-uniform range guard instead of one per quotient: the column holds the group's
      // round-0 values, each vouched for by its own lane (ok_ev0), so with out also in range
      // every numerator is 0 or in [2^-38, 2^38] and the packed Newton quotient is exact.
      if (__all(ok_ev0 && in_range19(out) && rt.ok)) {
        const pkf2 y2 = {rt.y, rt.y}, b2 = {rt.b, rt.b};
#pragma unroll
        for (int j = 0; j < N; j += 2) {
          const pkf2 q2 = fdiv_core_pk(pkf2{num[j], num[j + 1]}, b2, y2);
          row[j] = q2.x;
          row[j + 1] = q2.y;
        }
      } else {
#pragma unroll
        for (int j = 0; j < N; ++j) row[j] = fdiv_b(num[j], rt);
        if (!rt.ok) {
#pragma unroll
          for (int j = 0; j < N; ++j) row[j] = fdiv_ieee(num[j], rt.b);
        }
      }
      // tot = 0 (every peer's power on out's side of zero) is rare among 16 peers: one wave-uniform
      // test instead of 16 selects on every step
      if (__any(tot == 0.0f)) {
#pragma unroll
        for (int j = 0; j < N; ++j) row[j] = (tot == 0.0f) ? ev : row[j];
      }
    }
    soc = soc_r;

    // RC update and the next step's rows
    float tin1 = tin, tm1 = tm;
    rc_update(k, e0.t_out, hp, tin1, tm1);
    const StepIdx st1 = step_idx(w1, w2, tin1);
    uint64_t cw1 = code_word_t<TRAIN>(p, cw1r);
    if constexpr (kPair) {
      if (rng1) cw1 = (t1n & 1u) ? ((cw >> 32) | 0xFFFFFFFF00000000ull) : block2(t1n >> 1);
    }
    const uint32_t a0n = row0_addr(st1, cw1);
    const Row4<QT> row0n = gatq(a0n);
    const Row4<QT> rowNn = gatq(TRAIN ? st1.nrow : a0n);

    // the final P's column through the swizzled tile (community.py:45-54 needs P[j][i])
#pragma unroll
    for (int m = 0; m < 4; ++m)
      *reinterpret_cast<float4*>(tp + i * 16 + 4 * (m ^ (i & 3))) =
          make_float4(row[4 * m], row[4 * m + 1], row[4 * m + 2], row[4 * m + 3]);
    wave_lds_fence();
#pragma unroll
    for (int j = 0; j < N; ++j) col[j] = tp[j * 16 + cofs[j & 3]];
    wave_lds_fence();
    // ex = sign(pij) min(|pij|, |pji|) where the signs differ (community.py:48-50), one v_med3
    float g = 0.0f, pp = 0.0f;
#pragma unroll
    for (int j = 0; j < N; ++j) {
      const float pij = row[j], pji = col[j];
      const float ex = pair_exchange(pij, pji);
      g = g + (pij - ex);
      pp = pp + ex;
    }
    float cost = (g >= 0.0f) ? g * e0.buy : g * e0.inj;
    cost = cost + pp * e0.p2p;
    cost = fdiv_b(cost * k.slot, rmph);
    cost = cost * k.kilo;
    float pen = fmaxf(fmaxf(0.0f, k.lower - tin), fmaxf(0.0f, tin - k.upper));
    pen = pen > 0.0f ? pen + 1.0f : 0.0f;
    const float rw = -(cost + k.penw * pen);

    if constexpr (TRAIN) {
      if (active) {
        const QT qsa = sel3(act, rowR.v[0], rowR.v[1], rowR.v[2]);
        // alpha and gamma from LDS through an address the compiler cannot hoist: a broadcast LDS
        // read per step instead of four SGPRs held across the loop (spilled to VGPR lanes and read
        // back with v_readlane on the VALU)
        typedef __attribute__((address_space(3))) const double lds_double;
        uint32_t tdk_addr = (uint32_t)(uintptr_t)(lds_double*)tdk;
        asm volatile("" : "+s"(tdk_addr));
        lds_double* tdp = (lds_double*)(uintptr_t)tdk_addr;
        const double k_alpha = tdp[0], k_gamma = tdp[1];
        const double d = k_alpha * (((double)rw + k_gamma * (double)max3(rowN)) - (double)qsa);
        const long long dv = rne_ll(d * kDeltaScale);
#if P2PMG_SQ_ABL == 1
        if (dv == 0x7123456789LL)  // timing-only ablation: no hash insert (never true in practice)
#endif
        lds_add_by_key(hkey, hval, (st.strip + (uint32_t)ip) * kQPad + (uint32_t)act, dv, dbase);
      }
    }
    if constexpr (narrow) {
      *reinterpret_cast<float2*>(__builtin_assume_aligned(rec_ptr, 8)) = make_float2(rw, cost);
    } else {
      const uint32_t bins = ((uint32_t)st.it / 20u) | ((uint32_t)st.iT << 16);  // it * 400 + ib
      float4* rp = reinterpret_cast<float4*>(__builtin_assume_aligned(rec_ptr, 16));
      rp[0] = make_float4(rw, cost, g, pp);
      rp[1] = make_float4(tin, __uint_as_float(acts), __uint_as_float(bins), __uint_as_float(ips));
    }
    rec_ptr += rec_step;
    // avg_reward = sum_t mean_i r (community.py:179): the group's rewards in agent order
    tp[i] = rw;
    wave_lds_fence();
    float msum = 0.0f;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const float4 v = *reinterpret_cast<const float4*>(tp + 4 * m);
      msum = msum + v.x; msum = msum + v.y; msum = msum + v.z; msum = msum + v.w;
    }
    wave_lds_fence();
    ep_sum = ep_sum + div_n<N>(msum);
    if constexpr (TRAIN) {
      if (t % kSqFlushSteps == kSqFlushSteps - 1 || t + 1 == T)
        lds_hash_flush(hkey, hval, dbase, kSq16Waves * kWave);
    }

    tin = tin1;
    tm = tm1;
    w1 = w2;
    t2 = t2 + 1u == T32 ? 0u : t2 + 1u;
    st = st1;
    cw = cw1;
    a0 = a0n;
    row0 = row0n;
    rowN = rowNn;
  }
  if (active) {
    if (p.reset_t0)
      t0_draw(p.seed_lo, p.seed_hi, p.episode + 1, p.agent_offset + (uint32_t)a, p.setpoint, p.reset_sigma, tin, tm);
    p.t_in[a] = tin;
    p.t_m[a] = tm;
    if constexpr (BAT != 0) p.soc[a] = soc;
    if (i == 0) p.ep_reward[s] = ep_sum;
  }
}

template <typename QT, int R1, bool NARROW>
void launch_sq16_nw(const EpisodeParams& p, int blocks, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  const dim3 g(blocks), b(kWave * kSq16Waves);
  const int bat = !p.battery ? 0 : (p.bat_safe ? 2 : 1);
  if (p.mode == 0) {
    if (bat == 2) hipExtLaunchKernelGGL((episode_sq16_kernel<QT, R1, true, 2, NARROW>), g, b, 0, st, ev0, ev1, 0, p);
    else if (bat == 1) hipExtLaunchKernelGGL((episode_sq16_kernel<QT, R1, true, 1, NARROW>), g, b, 0, st, ev0, ev1, 0, p);
    else hipExtLaunchKernelGGL((episode_sq16_kernel<QT, R1, true, 0, NARROW>), g, b, 0, st, ev0, ev1, 0, p);
  } else {
    if (bat == 2) hipExtLaunchKernelGGL((episode_sq16_kernel<QT, R1, false, 2, NARROW>), g, b, 0, st, ev0, ev1, 0, p);
    else if (bat == 1) hipExtLaunchKernelGGL((episode_sq16_kernel<QT, R1, false, 1, NARROW>), g, b, 0, st, ev0, ev1, 0, p);
    else hipExtLaunchKernelGGL((episode_sq16_kernel<QT, R1, false, 0, NARROW>), g, b, 0, st, ev0, ev1, 0, p);
  }
}
template <typename QT, int R1>
void launch_sq16_r(const EpisodeParams& p, int blocks, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  if (p.rec_narrow) launch_sq16_nw<QT, R1, true>(p, blocks, ev0, ev1, st);
  else launch_sq16_nw<QT, R1, false>(p, blocks, ev0, ev1, st);
}
template <typename QT>
hipError_t launch_sq16_q(const EpisodeParams& p, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  const int waves = (p.S + kWave / 16 - 1) / (kWave / 16);
  const int blocks = (waves + kSq16Waves - 1) / kSq16Waves;
  if (p.R == 0) launch_sq16_r<QT, 1>(p, blocks, ev0, ev1, st);
  else if (p.R == 1) launch_sq16_r<QT, 2>(p, blocks, ev0, ev1, st);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

// sq16_prep_kernel: the policy-independent part of episode_sq16_kernel's per-step state, once per
// input upload (the runtime reruns it when env, profiles or max_in change): per (t, a) the agent's
// balance (load - pv) / max_in (agent.py:172-176, the IEEE quotient the kernel's guarded fast
// division returns) and the table offset of its time and balance bins, it * 8000 + ib * 20
// (rl.py:89-95 on the 20^4 table the sq16 path serves; the temperature bin is added in the kernel).
// The episode kernel then reads one 8-B word per agent-step instead of {load, pv} and skips the
// division and three of the four bins of every step.
__global__ void sq16_prep_kernel(const EpisodeParams p, uint2* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;  // k = t * A + a
  if (k >= (size_t)p.A * p.T) return;
  const int t = (int)(k / (size_t)p.A), a = (int)(k % (size_t)p.A);
  const int s_env = p.n_env == 1 ? 0 : a / p.N;
  const float time = p.env[((size_t)t * p.n_env + s_env) * kEnvStride];
  const float2 f = p.prof[k];
  const float bal = fdiv_ieee(f.x - f.y, p.max_in[a]);
  const int it = clamp_bin_f(time * 20.0f, 19.0f);
  const int ib = clamp_bin_f(((bal + 1.0f) / 2.0f) * 20.0f, 19.0f);
  out[k] = make_uint2(__float_as_uint(bal), (uint32_t)(it * 8000 + ib * 20));
}

}  // namespace

hipError_t launch_episode_sq16(const EpisodeParams& p, int q_dtype, hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream) {
  return q_dtype == 0 ? launch_sq16_q<double>(p, ev0, ev1, stream) : launch_sq16_q<float>(p, ev0, ev1, stream);
}

hipError_t launch_sq16_prep(const EpisodeParams& p, uint2* out, hipStream_t stream) {
  const size_t n = (size_t)p.A * p.T;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(sq16_prep_kernel, dim3(grid_for(n, 256)), dim3(256), 0, stream, p, out);
  return hipGetLastError();
}

}  // namespace p2pmg
