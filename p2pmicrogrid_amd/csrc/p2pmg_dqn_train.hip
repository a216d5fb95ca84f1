// p2pmg_dqn_train.hip — the DQN train kernel (Trainer._train / _soft_update rl.py:307-359; the env step
// and the layouts: p2pmg_dqn_act.hip):
//   dqn_train_kernel     one 4-wave workgroup per agent (or per run of agents when the network
//                        is shared): samples 32 transitions, target forward over the 96 rows
//                        (ns x 3 action values), online forward + backward over the 32 rows, all
//                        on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation); wave w
//                        owns hidden units 16w..16w+15 of both 64-wide layers (layer 2 as the
//                        transposed product, so layer 3 reduces in-lane).  Per-agent
//                        networks: clip + Adam + soft update fused in the epilogue; shared: the
//                        workgroup's gradient sum is written as a partial.
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {
#include "p2pmg_device.h"
#include "p2pmg_dqn_ops.h"
#include "p2pmg_dqn_step.h"

constexpr int kLdsRowT = 48;  // H1oT rows (32 data rows + pad): 16 units x 4 k of one read hit 64 banks

// ----------------------------------------------------------------- train: Trainer._train
// hyp: the network's own {gamma, tau, tau_c, clip} (wave-uniform)
__device__ __forceinline__ void adam_update(const DqnParams& d, float4 hyp, float* th, float* tg, float* mm, float* vv,
                                            int idx, float g, float lr) {
  // Keras Adam then Trainer._soft_update (rl.py:335-354), in place
  const AdamStep s = adam_step(d, mm[idx], vv[idx], th[idx], g, lr);
  mm[idx] = s.m;
  vv[idx] = s.v;
  th[idx] = s.w;
  tg[idx] = soft_update(hyp.y, hyp.z, tg[idx], s.w);
}

// one thread's share of agent a's sampled batch (thread t: sample t / 8, floats t % 8 and, for
// t % 8 < 2, t % 8 + 8), gathered from the replay ring through the sample kernel's slot indices
// (a is uniform: the agent's ring and slot row are scalar bases, each lane adds a 32-bit byte offset,
// so no per-lane 64-bit address stays live across the agent loop)
__device__ __forceinline__ int batch_slot(const DqnParams& d, int a, int t) {
  const char* row = reinterpret_cast<const char*>(d.smp) + (size_t)a * kB * sizeof(int);
  return *reinterpret_cast<const int*>(row + (uint32_t)(t >> 3) * (uint32_t)sizeof(int));
}
__device__ __forceinline__ void batch_part_at(const DqnParams& d, int a, int t, int slot, float& v0, float& v1) {
  const int k = t & 7;
  const char* ring = reinterpret_cast<const char*>(d.buf + (size_t)a * d.cap * kTrans);
  const uint32_t off = ((uint32_t)slot * kTrans + (uint32_t)k) * (uint32_t)sizeof(float);  // cap * 40 B < 4 GiB
  v0 = *reinterpret_cast<const float*>(ring + off);
  v1 = k < kTrans - 8 ? *reinterpret_cast<const float*>(ring + off + 8 * sizeof(float)) : 0.0f;
}
__device__ __forceinline__ void batch_part(const DqnParams& d, int a, int t, float& v0, float& v1) {
  batch_part_at(d, a, t, batch_slot(d, a, t), v0, v1);
}
__device__ __forceinline__ void batch_put(float* dst, int t, float v0, float v1) {
  const int b = t >> 3, k = t & 7;
  dst[b * kTrans + k] = v0;
  if (k < kTrans - 8) dst[b * kTrans + k + 8] = v1;
}

// the weights one train workgroup reads, per lane (layer 1 and dH1: column col of wave w;
// layers 2 and 3: the 4 hidden units 16 w + 4 g4 + r of the transposed tiles).  Per-agent networks
// read W2 per MFMA step from L1/L2; a shared network keeps its 48 W2 operands in registers.
struct TrainW {
  float bt0, bo0, bo1, b1t, b1o, b3t, b3o, w14t;  // layer 1: W1[g4][col], W1[4][col] (g4 = 0), biases
  float b2t[4], w3t[4], b2o[4], w3o[4];  // layer 2/3 of the hidden units 16 w + 4 g4 + r
};
__device__ __forceinline__ void load_train_w(TrainW& W, const float* th, const float* tg, int col, int g4, int h0) {
  W.bt0 = tg[kOffW1 + g4 * kH + col];
  W.bo0 = th[kOffW1 + g4 * kH + col];
  W.w14t = tg[kOffW1 + 4 * kH + col];
  W.bo1 = g4 == 0 ? th[kOffW1 + 4 * kH + col] : 0.0f;
  W.b1t = tg[kOffB1 + col];
  W.b1o = th[kOffB1 + col];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    W.b2t[r] = tg[kOffB2 + h0 + r];
    W.w3t[r] = tg[kOffW3 + h0 + r];
    W.b2o[r] = th[kOffB2 + h0 + r];
    W.w3o[r] = th[kOffW3 + h0 + r];
  }
  W.b3t = tg[kOffB3];
  W.b3o = th[kOffB3];
}

// timing-only probe (-DP2PMG_TRACE, P2PMG_STAMP): per-phase splits of the agent loop, printed for env
// step 50 by every wave of two workgroups (scripts/gpu_dqn_trace.sh).  A phase's time includes
// the other workgroup's MFMAs sharing the SIMD, and MFMA results landing after their issue.
//
// train workgroups per CU (waves per SIMD): 2 in the default build (about 220 VGPRs)
#ifndef P2PMG_TRAIN_OCC
#define P2PMG_TRAIN_OCC 2
#endif
// ROLES (with SHARED): one network per role (p2pmg_dqn_setup_roles).  Workgroup role * bps + j chains the
// batch gradients of agents (j apb + ag) N + role, the role's agents in scenario order, against network
// `role`, whose W2 operands it holds in registers as the shared form holds network 0's, and writes the
// partial [role][j] for dqn_reduce_adam_kernel<true>.
template <bool SHARED, bool ROLES = false>
__global__ __launch_bounds__(256, P2PMG_TRAIN_OCC) void dqn_train_kernel(const DqnParams d) {
  static_assert(SHARED || !ROLES, "the role form writes partials");
  __shared__ float smpb[2][kB * kTrans];  // this agent's batch and the next one's (prefetched)
  __shared__ float H1t[3 * kB][kLdsRow];
  __shared__ __attribute__((aligned(16))) float H1oT[kH][kLdsRowT];  // online layer-1 activations, unit-major
  __shared__ __attribute__((aligned(16))) float dZ2[kB][kLdsRow];
  __shared__ float qpart[4][4 * kB];  // per-wave partial Q: rows 0..95 target (action x sample), 96..127 online
  const EpisodeParams& p = d.e;
  const int w = threadIdx.x / kWave, l = threadIdx.x % kWave;
  const int c16 = l & 15, g4 = l >> 4;
  const int col = 16 * w + c16;     // this lane's column of layer 1 and of dH1
  const int h0 = 16 * w + 4 * g4;   // this lane's 4 hidden units of layer 2 (transposed tiles)
  const size_t A = (size_t)p.A;

  f32x4 gW2[4], gW1[2];
#pragma unroll
  for (int m = 0; m < 4; ++m) gW2[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  gW1[0] = gW1[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  float gx1[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float gb1 = 0.0f, gb3 = 0.0f;
  float gb2[4] = {0.0f, 0.0f, 0.0f, 0.0f}, gW3[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  // this workgroup's run of agents: block j of gradient segment g covers agents g * seg_agents +
  // j * apb .. (clipped to the segment), so no block straddles two segments (p2pmg_dqn_config)
  // (role form: seg is the role, its agents are a_step = N apart and end at scenario S - 1)
  const int seg = blockIdx.x / d.bps, sblk = blockIdx.x - seg * d.bps;
  const int a_step = ROLES ? d.roles : 1;
  const int a_first = ROLES ? sblk * d.apb * d.roles + seg : seg * d.seg_agents + sblk * d.apb;
  const int n_ag = ROLES ? max(0, min(d.apb, p.S - sblk * d.apb))
                         : (d.batch ? 1 : max(0, min(d.apb, (seg + 1) * d.seg_agents - a_first)));
  int net = ROLES ? seg : (d.batch ? d.net : 0);
  // the workgroup's network's {gamma, tau, tau_c, clip}: per-agent networks train one agent per workgroup,
  // so its row (d.hyp, when the networks' constants differ) is one scalar load from a uniform address,
  // and the four values stay SGPRs like the kernel arguments they stand in for
  const int net_h = __builtin_amdgcn_readfirstlane(ROLES ? seg : (d.batch ? d.net : (SHARED ? 0 : a_first)));
  const float4 hyp = d.hyp ? d.hyp[net_h] : make_float4(d.gamma, d.tau, d.tau_c, d.clip);
  TrainW W;
  // one shared network: the lane's 48 W2 operands (layer 2: W2[4 kk + g4][col] of the target and
  // the online network; dH1: W2[col][4 kk + g4]) stay in registers for the whole launch
  float w2t[SHARED ? 16 : 1], w2o[SHARED ? 16 : 1], w2c[SHARED ? 16 : 1];
  if constexpr (SHARED) {
    const float* th0 = d.theta + (size_t)net * kNetStride;
    const float* tg0 = d.target + (size_t)net * kNetStride;
    load_train_w(W, th0, tg0, col, g4, h0);
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      w2t[kk] = tg0[kOffW2 + (4 * kk + g4) * kH + col];
      w2o[kk] = th0[kOffW2 + (4 * kk + g4) * kH + col];
      w2c[kk] = th0[kOffW2 + col * kH + 16 * g4 + kk];  // dH1's K order: unit 16 g4 + kk
    }
  }
  // the first agent's batch (explicit batch, or the sample pre-pass output)
  if (d.batch) {
    for (int k = threadIdx.x; k < kB * kTrans; k += 256) smpb[0][k] = d.batch[k];
  } else {
    float v0 = 0.0f, v1 = 0.0f;
    if (n_ag > 0) batch_part(d, a_first, threadIdx.x, v0, v1);
    batch_put(smpb[0], threadIdx.x, v0, v1);
  }
  // the next agent's slot index, loaded one agent ahead of its transitions: the dependent pair of
  // loads never makes the loop wait for a global round trip
  // (unconditional loads at clamped in-range indices: a branch around them would leave a
  // loop-carried register copy that waits for every load in flight)
  const int a_last = ROLES ? (int)A - d.roles + seg : (int)A - 1;  // the role's last agent: the clamp stays in its run
  const int tag4 = reduce4_tag();
  int slot_n = batch_slot(d, min(a_first + a_step, a_last), threadIdx.x);
  __syncthreads();

#if P2PMG_TRACE
  uint64_t trp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast;
  asm volatile("s_memtime %0\n s_waitcnt lgkmcnt(0)" : "=s"(tlast)::"memory");
#endif
  for (int ag = 0; ag < n_ag; ++ag) {
    const int a = ROLES ? a_first + ag * a_step : (d.batch ? 0 : a_first + ag);
    net = ROLES ? seg : (d.batch ? d.net : (SHARED ? 0 : a));
    const float* th = d.theta + (size_t)net * kNetStride;
    const float* tg = d.target + (size_t)net * kNetStride;
    if (!SHARED) load_train_w(W, th, tg, col, g4, h0);
    float (*smp)[kTrans] = reinterpret_cast<float (*)[kTrans]>(smpb[ag & 1]);
    // prefetch the next agent's batch into registers; it goes to the other buffer at the end
    const bool has_next = !d.batch && ag + 1 < n_ag;
    float nx0, nx1;
    batch_part_at(d, min(a + a_step, a_last), threadIdx.x, (int)min((unsigned)slot_n, (unsigned)(d.cap - 1)), nx0, nx1);
    slot_n = batch_slot(d, min(a + 2 * a_step, a_last), threadIdx.x);

    // ---- layer 1: Z1 = X W1 + b1, 6 target + 2 online row tiles (K = 4 on MFMA, the action term
    // K = 4 as an fmaf for target tiles, a second MFMA for online tiles)
    const float bt0 = W.bt0, bo0 = W.bo0, bo1 = W.bo1, b1t = W.b1t, b1o = W.b1o;
    unsigned z1mask = 0;  // online rows where z1 > 0 (ReLU derivative), bit 4 rt + r
    __builtin_amdgcn_s_setprio(2);  // MFMA phase (see layer 2)
    // all products first (8 independent accumulators), then the bias / ReLU / LDS stores: no store
    // waits on the MFMA it follows
    f32x4 z1[8];
#pragma unroll
    for (int rt = 0; rt < 6; ++rt) {
      const int b = (16 * rt + c16) % kB;
      z1[rt] = mfma4(smp[b][6 + g4], bt0, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
    }
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) z1[6 + rt] = mfma4(smp[16 * rt + c16][g4], bo0, f32x4{0.0f, 0.0f, 0.0f, 0.0f});
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) z1[6 + rt] = mfma4(g4 == 0 ? smp[16 * rt + c16][4] : 0.0f, bo1, z1[6 + rt]);
    // a target tile holds one action value (rows 16 rt .. + 15: action rt / 2), so its K = 4 term
    // is a per-column fmaf, the same single rounding as an MFMA's second product would give
#pragma unroll
    for (int rt = 0; rt < 6; ++rt)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        H1t[16 * rt + 4 * g4 + r][col] = relu(fmaf((rt >> 1) == 0 ? 0.0f : ((rt >> 1) == 1 ? 0.5f : 1.0f), W.w14t, z1[rt][r]) + b1t);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      float h[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = z1[6 + rt][r] + b1o;
        h[r] = relu(z);
        if (z > 0.0f) z1mask |= 1u << (4 * rt + r);
      }
      *reinterpret_cast<float4*>(&H1oT[col][16 * rt + 4 * g4]) = make_float4(h[0], h[1], h[2], h[3]);
    }
    __builtin_amdgcn_s_setprio(0);
    P2PMG_STAMP(trp, tlast, 0);
    __syncthreads();
    P2PMG_STAMP(trp, tlast, 1);

    // The MFMA phases (layers 1 and 2, the backward products) run at raised wave priority: the
    // SIMD's other wave (another workgroup, in a VALU / LDS phase) then issues into the MFMA shadow
    // instead of competing with the MFMA stream (configs[4] 14.55 -> 13.93 ms per episode)
    __builtin_amdgcn_s_setprio(2);
    // ---- layer 2 as Z2^T = W2^T H1^T (K = 64): the operands of H1 W2 with the MFMA's A and B
    // swapped, so the accumulator of row tile rt holds data row 16 rt + c16 at the hidden units
    // h0 + r.  Layer 3 then sums 4 units in-lane and the 4 row groups with two exchanges, instead
    // of a 16-lane butterfly per (row, unit).
    f32x4 at[6], ao[2];
#pragma unroll
    for (int rt = 0; rt < 6; ++rt) at[rt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    ao[0] = ao[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      const int k = 4 * kk + g4;
      const float bt = SHARED ? w2t[SHARED ? kk : 0] : tg[kOffW2 + k * kH + col];
      const float bo = SHARED ? w2o[SHARED ? kk : 0] : th[kOffW2 + k * kH + col];
#pragma unroll
      for (int rt = 0; rt < 6; ++rt) at[rt] = mfma4(bt, H1t[16 * rt + c16][k], at[rt]);
      ao[0] = mfma4(bo, H1oT[k][c16], ao[0]);
      ao[1] = mfma4(bo, H1oT[k][16 + c16], ao[1]);
    }
    __builtin_amdgcn_s_setprio(0);
    P2PMG_STAMP(trp, tlast, 2);
    // ---- layer 3, this wave's 16 units: in-lane over r (a pairwise tree), then over the 4 row
    // groups for four tiles at once (reduce4_groups: 3 lane swaps + 3 adds, row group g4 ends with
    // tile tag4's sum), so every lane stores one value per four tiles, without a masked branch
    float s8[8];
#pragma unroll
    for (int rt = 0; rt < 6; ++rt) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = relu(at[rt][r] + W.b2t[r]) * W.w3t[r];
      s8[rt] = (v[0] + v[1]) + (v[2] + v[3]);
    }
    float h2o[2][4];
    unsigned z2mask = 0;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      float v[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float z = ao[rt][r] + W.b2o[r];
        h2o[rt][r] = relu(z);
        if (z > 0.0f) z2mask |= 1u << (4 * rt + r);
        v[r] = h2o[rt][r] * W.w3o[r];
      }
      s8[6 + rt] = (v[0] + v[1]) + (v[2] + v[3]);
    }
    qpart[w][16 * tag4 + c16] = reduce4_groups(s8[0], s8[1], s8[2], s8[3]);
    qpart[w][4 * kB / 2 + 16 * tag4 + c16] = reduce4_groups(s8[4], s8[5], s8[6], s8[7]);
    P2PMG_STAMP(trp, tlast, 3);
    __syncthreads();
    P2PMG_STAMP(trp, tlast, 1);

    // ---- targets y = r + gamma * max_a' Q_target(ns, a') and dL/dq (rl.py:314-331), for this
    // lane's data rows b = 16 rt + c16
    float dq[2];
    float lsum = 0.0f, dqsum = 0.0f;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      const int b = 16 * rt + c16;
      float qt[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int row = k * kB + b;
        qt[k] = (((qpart[0][row] + qpart[1][row]) + qpart[2][row]) + qpart[3][row]) + W.b3t;
      }
      const int ro = 3 * kB + b;
      const float q = (((qpart[0][ro] + qpart[1][ro]) + qpart[2][ro]) + qpart[3][ro]) + W.b3o;
      const float y = smp[b][5] + hyp.x * fmaxf(fmaxf(qt[0], qt[1]), qt[2]);
      const float diff = q - y;
      dq[rt] = (2.0f / (float)kB) * diff;
      lsum += diff * diff;
      dqsum += dq[rt];
    }
    // the 16 lanes of a row group hold the 32 rows: dL/db3 = sum dq in wave 0, the loss
    // mean (y - q)^2 (only when it is recorded) in wave 1, so neither holds the others at the barrier
    if (w == 0) {
      const float dqs = sum16(dqsum);
      if (l == 0) gb3 += dqs;
    } else if (w == 1 && (d.batch || d.rec_loss)) {
      const float ls = sum16(lsum);
      if (l == 0) {
        const float loss = ls / (float)kB;
        if (d.batch) d.loss_out[0] = loss;
        else d.rec_loss[(size_t)d.t * A + a] = loss;
      }
    }

    // ---- backward: dZ2 of this lane's (row, units), stored row-major for dW2 and dH1
#pragma unroll
    for (int rt = 0; rt < 2; ++rt) {
      float dz2[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool on = (z2mask >> (4 * rt + r)) & 1u;
        dz2[r] = on ? dq[rt] * W.w3o[r] : 0.0f;
        gW3[r] += h2o[rt][r] * dq[rt];
        gb2[r] += dz2[r];
      }
      *reinterpret_cast<float4*>(&dZ2[16 * rt + c16][h0]) = make_float4(dz2[0], dz2[1], dz2[2], dz2[3]);
    }
    P2PMG_STAMP(trp, tlast, 4);
    __syncthreads();
    P2PMG_STAMP(trp, tlast, 1);
    __builtin_amdgcn_s_setprio(2);
    // Every operand of the backward products is read from LDS up front (16-B reads where the K
    // order allows), so the MFMA chains below never wait on a read between two products.
    // dW2 = H1^T dZ2 over the 32 data rows in the K order b = 8 g4 + q: A = H1oT[16 mt + c16][b]
    // (two 16-B reads per mt), B = dZ2[b][col]; accumulator rows = layer-1 units 16 mt + 4 g4 + r,
    // columns = the wave's layer-2 units col
    float ha[4][8], db[8];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const float4 u0 = *reinterpret_cast<const float4*>(&H1oT[16 * mt + c16][8 * g4]);
      const float4 u1 = *reinterpret_cast<const float4*>(&H1oT[16 * mt + c16][8 * g4 + 4]);
      ha[mt][0] = u0.x; ha[mt][1] = u0.y; ha[mt][2] = u0.z; ha[mt][3] = u0.w;
      ha[mt][4] = u1.x; ha[mt][5] = u1.y; ha[mt][6] = u1.z; ha[mt][7] = u1.w;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) db[q] = dZ2[8 * g4 + q][col];
    // dH1 = dZ2 W2^T (own columns n = col) in the K order unit 16 g4 + kk: A = dZ2[16 rt + c16][16 g4
    // .. + 15] (four 16-B reads per rt), B = W2[col][16 g4 + kk] (registers for a shared network)
#if P2PMG_TRAIN_OCC >= 3  // register budget: dW2's products issue before dH1's operands are read
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) gW2[mt] = mfma4(ha[mt][q], db[q], gW2[mt]);
    __builtin_amdgcn_sched_barrier(0);
#endif
    float za[2][16];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float4 u = *reinterpret_cast<const float4*>(&dZ2[16 * rt + c16][16 * g4 + 4 * v]);
        za[rt][4 * v] = u.x; za[rt][4 * v + 1] = u.y; za[rt][4 * v + 2] = u.z; za[rt][4 * v + 3] = u.w;
      }
    // dW1's A operand: input feature c16 (< 5) of data rows b = 16 rt + 4 g4 + r (lanes c16 >= 5 read
    // feature 4 and select 0: no exec-masked read)
#if P2PMG_TRAIN_OCC < 3
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) gW2[mt] = mfma4(ha[mt][q], db[q], gW2[mt]);
#endif
    f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
        acc[rt] = mfma4(za[rt][kk], SHARED ? w2c[SHARED ? kk : 0] : th[kOffW2 + col * kH + 16 * g4 + kk], acc[rt]);
    // dZ1 = dH1 * [z1 > 0]; dW1 = X^T dZ1 (two accumulators: independent chains)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt) {
        const float dz1 = ((z1mask >> (4 * rt + r)) & 1u) ? acc[rt][r] : 0.0f;
        gb1 += dz1;
        // dW1 = X^T dZ1 on VALU: this lane's partial over its 8 data rows, reduced over the row
        // groups once per launch (5 useful output rows of 16 made the MFMA form mostly padding)
        const float* xr = smp[16 * rt + 4 * g4 + r];
#pragma unroll
        for (int k = 0; k < 5; ++k) gx1[k] = fmaf(xr[k], dz1, gx1[k]);
      }
    __builtin_amdgcn_s_setprio(0);
    if (has_next) batch_put(smpb[(ag + 1) & 1], threadIdx.x, nx0, nx1);
    P2PMG_STAMP(trp, tlast, 5);
    __syncthreads();  // every wave is done with this agent's LDS and with the online W2
    P2PMG_STAMP(trp, tlast, 1);
  }
#if P2PMG_TRACE
  if (l == 0 && (blockIdx.x == 0 || blockIdx.x == gridDim.x / 2) && !d.batch && d.t == 50)
    printf("DQNTRACE blk %d wave %d agents %d, cycles per agent: layer1 %.0f layer2 %.0f layer3 %.0f "
           "targets+dz2 %.0f backward %.0f barrier waits %.0f\n",
           (int)blockIdx.x, w, n_ag, (double)trp[0] / n_ag, (double)trp[2] / n_ag, (double)trp[3] / n_ag,
           (double)trp[4] / n_ag, (double)trp[5] / n_ag, (double)trp[1] / n_ag);
#endif

  gb1 = sum_groups(gb1);
  float g1t[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) g1t[k] = sum_groups(gx1[k]);
  // lane (g4, r) owns dW1 row 4 g4 + r (< 5): g4 = 0 rows 0..3, g4 = 1 row 4
  auto dw1 = [&](int r) { return g4 == 0 ? g1t[r] : g1t[4]; };
#pragma unroll
  for (int r = 0; r < 4; ++r) {  // over the 16 data-row lanes of each row group
    gb2[r] = sum16(gb2[r]);
    gW3[r] = sum16(gW3[r]);
  }
  const int net_out = net;
  if constexpr (!SHARED) {
    // Trainer._train epilogue: clip the first kernel's gradient, Adam, then update_targets
    float* th = d.theta + (size_t)net_out * kNetStride;
    float* tg = d.target + (size_t)net_out * kNetStride;
    float* mm = d.adam_m + (size_t)net_out * kNetStride;
    float* vv = d.adam_v + (size_t)net_out * kNetStride;
    // each DQNAgent has its own Adam (agent.py:310): its own iteration count, so its own step size
    const float lr = d.lr_net ? d.lr_net[net_out] : d.lr_t;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) adam_update(d, hyp, th, tg, mm, vv, kOffW2 + (16 * mt + 4 * g4 + r) * kH + col, gW2[mt][r], lr);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 4 * g4 + r;
      if (k < 5) adam_update(d, hyp, th, tg, mm, vv, kOffW1 + k * kH + col, fminf(fmaxf(dw1(r), -hyp.w), hyp.w), lr);
    }
    if (g4 == 0) adam_update(d, hyp, th, tg, mm, vv, kOffB1 + col, gb1, lr);
    if (c16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        adam_update(d, hyp, th, tg, mm, vv, kOffB2 + h0 + r, gb2[r], lr);
        adam_update(d, hyp, th, tg, mm, vv, kOffW3 + h0 + r, gW3[r], lr);
      }
    }
    if (threadIdx.x == 0) adam_update(d, hyp, th, tg, mm, vv, kOffB3, gb3, lr);
  } else {
    float* gp = d.grad + (size_t)blockIdx.x * kNetStride;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) gp[kOffW2 + (16 * mt + 4 * g4 + r) * kH + col] = gW2[mt][r];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * g4 + r < 5) gp[kOffW1 + (4 * g4 + r) * kH + col] = dw1(r);
    if (g4 == 0) gp[kOffB1 + col] = gb1;
    if (c16 == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gp[kOffB2 + h0 + r] = gb2[r];
        gp[kOffW3 + h0 + r] = gW3[r];
      }
    }
    if (threadIdx.x == 0) gp[kOffB3] = gb3;
  }
}

}  // namespace

int dqn_train_blocks_per_cu() { return P2PMG_TRAIN_OCC; }

hipError_t launch_dqn_train(const DqnParams& d, int blocks, bool shared_partials, hipStream_t st) {
  if (shared_partials)
    hipLaunchKernelGGL(dqn_train_kernel<true>, dim3(blocks), dim3(256), 0, st, d);
  else
    hipLaunchKernelGGL(dqn_train_kernel<false>, dim3(blocks), dim3(256), 0, st, d);
  return hipGetLastError();
}

hipError_t launch_dqn_train_roles(const DqnParams& d, hipStream_t st) {
  if (d.roles < 1 || d.bps < 1 || d.apb < 1 || d.batch || d.e.A != d.e.S * d.roles ||
      (long long)d.bps * d.apb < d.e.S)  // every scenario in a block, no agent past A
    return hipErrorInvalidValue;
  hipLaunchKernelGGL((dqn_train_kernel<true, true>), dim3(d.roles * d.bps), dim3(256), 0, st, d);
  return hipGetLastError();
}

}  // namespace p2pmg
