// p2pmg_dqn_map.hip — gfx950 kernels of the DQN policy map (p2pmg_dqn_policy_map, p2pmg_dqn_map_stats,
// p2pmg_dqn_policy_mark, p2pmg_dqn_policy_changes): the Q-MLP of every network evaluated at every state
// of a rectangular grid of observations and at the three action values, so that one byte per state,
// eight numbers or one count per network reach the host (ActorModel.greedy_action rl.py:188-196 over
// the state grid of data_analysis.py's plot_q_values_* / compare_decisions*).  A post-pass: it reads the
// weights where they lie and changes no episode kernel.
//
//   dqn_map_kernel<CMP>   one 4-wave workgroup works on ONE network (net = blockIdx / bpn) and strides
//                         over that network's passes of kPass = 64 states (4 tiles of 16 states x 3
//                         actions = 192 rows) by bpn.  Per (block, network), once: the W2 operands, b2, w3
//                         (registers, dqn_act_shared_kernel's layout), the layer-1 column of unit = lane,
//                         and the grid axes (LDS).  Per pass:
//                           wave 3   decomposes the NEXT pass's 64 state indices into (i0..i3) and writes
//                                    their observations to LDS (states past the range recompute its last
//                                    state and are masked out of every result);
//                           layer 1  VALU, wave w = tile w, lane = hidden unit: p2p W1[3], fmaf balance,
//                                    temp, time; the three action forms; relu -> H1 (LDS, padded rows);
//                           layer 2  Z2^T = W2^T H1^T on v_mfma_f32_16x16x4_f32, k ascending from a zero
//                                    accumulator, wave w owning units 16w .. 16w+15, 12 accumulators;
//                           layer 3  4 units in-lane, the 4 row groups (reduce4_groups), the 4 waves
//                                    pairwise, + b3: wave_sum's tree, the act kernels' bits;
//                           wave 0   lane = state: first-maximum argmax, extrema, counts, the byte (four
//                                    lanes' bytes in one dword store where every network's bytes start
//                                    4-byte aligned), the Q values, the snapshot compare (CMP).
//   dqn_map_fold_kernel   one wave per network folds the [bpn] block partials.
// Every statistic is a count, a minimum or a maximum: no atomics, no dependence on the launch shape.
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {
#include "p2pmg_device.h"
#include "p2pmg_dqn_ops.h"

constexpr int kBlock = 256;               // 4 waves
constexpr int kTP = 4;                    // 16-state tiles per pass (one per wave in layer 1)
constexpr int kPass = 16 * kTP;           // states per pass: wave 0 finishes one per lane
constexpr int kMT = 3 * kTP;              // MFMA row tiles per pass (tile tp, action a: 3 tp + a)
constexpr unsigned kResident = 512;       // 256 CUs x 2 workgroups (LDS and the launch bound)
constexpr uint32_t kAxesLds = 1024;       // axis values held in LDS (more: read through L2)

// store byte b of every valid lane at dst[i]; dword: i of lane 4k is a multiple of 4 and states
// i .. i + 3 are valid together, so lane 4k stores the four bytes of lanes 4k .. 4k + 3
__device__ __forceinline__ void store_bytes(uint8_t* dst, size_t i, bool valid, uint32_t b, bool dword) {
  if (dword) {
    // within each quad: lane i takes lane i + 1's byte, then lane i + 2's half (DPP quad_perm [1,2,3,3], [2,3,2,3])
    const uint32_t w1 = b | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0xF9, 0xF, 0xF, false) << 8);
    const uint32_t w = w1 | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)w1, 0xEE, 0xF, 0xF, false) << 16);
    if (valid && (threadIdx.x & 3u) == 0u) *reinterpret_cast<uint32_t*>(dst + i) = w;
  } else if (valid) {
    dst[i] = (uint8_t)b;
  }
}

template <bool CMP>
__global__ __launch_bounds__(kBlock, 2) void dqn_map_kernel(const DqnMapParams p) {
  __shared__ float H1[16 * kMT][kLdsRow];
  __shared__ float qpart[4][kTP][64];  // [wave][tile][16 x action (reduce4_tag) + slot]
  __shared__ float4 shX[kPass];        // time, temp, balance, p2p of the pass's state slot
  __shared__ float shAx[kAxesLds];
  const int tid = threadIdx.x;
  const int w = tid / kWave, l = tid % kWave;
  const int c16 = l & 15, g4 = l >> 4;
  const unsigned net = blockIdx.x / p.bpn, blk = blockIdx.x - net * p.bpn;
  const float* th = p.theta + (size_t)net * kNetStride;
  const uint32_t n1 = p.n[1], n2 = p.n[2], n3 = p.n[3];
  const uint32_t o1 = p.n[0], o2 = o1 + n1, o3 = o2 + n2, n_ax = o3 + n3;  // axis offsets in p.axes
  const uint32_t g_last = p.g_begin + p.g_count - 1;
  const uint32_t n_pass = (p.g_count + kPass - 1) / kPass;

  // layer 1 (lane = hidden unit u): W1 column and b1
  const int u = l;
  const float w10 = th[kOffW1 + 0 * kH + u], w11 = th[kOffW1 + 1 * kH + u], w12 = th[kOffW1 + 2 * kH + u],
              w13 = th[kOffW1 + 3 * kH + u], w14 = th[kOffW1 + 4 * kH + u], b1 = th[kOffB1 + u];
  // layer 2 / 3 (wave w, lane: A operand W2[4 kk + g4][16 w + c16]; accumulator units 16 w + 4 g4 + r)
  float w2[16];
#pragma unroll
  for (int kk = 0; kk < 16; ++kk) w2[kk] = th[kOffW2 + (4 * kk + g4) * kH + 16 * w + c16];
  float b2[4], w3[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    b2[r] = th[kOffB2 + 16 * w + 4 * g4 + r];
    w3[r] = th[kOffW3 + 16 * w + 4 * g4 + r];
  }
  const float b3 = th[kOffB3];
  const int tag4 = reduce4_tag();

  const bool ax_lds = n_ax <= kAxesLds;
  if (ax_lds)
    for (uint32_t k = tid; k < n_ax; k += kBlock) shAx[k] = p.axes[k];
  __syncthreads();
  // the observation of state slot l of pass ps (wave 3): g = ((i0 n1 + i1) n2 + i2) n3 + i3
  auto stage_obs = [&](uint32_t ps) {
    uint32_t g = p.g_begin + ps * kPass + (uint32_t)l;
    g = g < g_last ? g : g_last;
    const uint32_t r3 = g / n3, i3 = g - r3 * n3;
    const uint32_t r2 = r3 / n2, i2 = r3 - r2 * n2;
    const uint32_t i0 = r2 / n1, i1 = r2 - i0 * n1;
    float4 x;
    if (ax_lds) x = make_float4(shAx[i0], shAx[o1 + i1], shAx[o2 + i2], shAx[o3 + i3]);
    else x = make_float4(p.axes[i0], p.axes[o1 + i1], p.axes[o2 + i2], p.axes[o3 + i3]);
    shX[l] = x;
  };
  if (w == 3 && blk < n_pass) stage_obs(blk);
  __syncthreads();

  // wave 0, lane = state slot: the block's running results
  float lo = __builtin_inff(), hi = -__builtin_inff(), gap = __builtin_inff();
  uint32_t n_g0 = 0, n_g1 = 0, n_g2 = 0, n_chg = 0;
  const size_t row = (size_t)net * p.g_count;  // this network's first byte of policy / snap, first Q triple
  const bool dword = p.dword != 0;

  for (uint32_t ps = blk; ps < n_pass; ps += p.bpn) {
    // layer 1: the three action rows of tile w's 16 states at unit u
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float4 x = shX[16 * w + q];
      float z = x.w * w13;
      z = fmaf(x.z, w12, z);
      z = fmaf(x.y, w11, z);
      z = fmaf(x.x, w10, z);
      H1[16 * (3 * w + 0) + q][u] = relu(z + b1);
      H1[16 * (3 * w + 1) + q][u] = relu(fmaf(0.5f, w14, z) + b1);
      H1[16 * (3 * w + 2) + q][u] = relu((z + w14) + b1);
    }
    __syncthreads();
    if (w == 3 && ps + p.bpn < n_pass) stage_obs(ps + p.bpn);  // every read of shX is behind the barrier
    f32x4 acc[kMT];
#pragma unroll
    for (int m = 0; m < kMT; ++m) acc[m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
      for (int m = 0; m < kMT; ++m) acc[m] = mfma4(w2[kk], H1[16 * m + c16][4 * kk + g4], acc[m]);
#pragma unroll
    for (int tp = 0; tp < kTP; ++tp) {
      float sq[3];
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = relu(acc[3 * tp + a][r] + b2[r]) * w3[r];
        sq[a] = (v[0] + v[1]) + (v[2] + v[3]);  // wave_sum's tree: 4 units in-lane, ...
      }
      qpart[w][tp][16 * tag4 + c16] = reduce4_groups(sq[0], sq[1], sq[2], 0.0f);  // ... the 4 row groups
    }
    __syncthreads();
    if (w == 0) {
      const uint32_t gu = ps * kPass + (uint32_t)l;  // state of this lane, relative to g_begin
      const bool valid = gu < p.g_count;
      const uint32_t gr = valid ? gu : p.g_count - 1;
      float qv[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int s = 16 * k + c16;
        qv[k] = ((qpart[0][g4][s] + qpart[1][g4][s]) + (qpart[2][g4][s] + qpart[3][g4][s])) + b3;  // ... the 4 waves
      }
      // ActorModel.greedy_action rl.py:188-196: argmax over (0, .5, 1), first maximum
      uint32_t act = 0;
      float best = qv[0];
      if (qv[1] > best) { best = qv[1]; act = 1; }
      if (qv[2] > best) { best = qv[2]; act = 2; }
      const float o0 = act == 0 ? qv[1] : qv[0], o1v = act == 2 ? qv[1] : qv[2];
      const float d = best - (o0 > o1v ? o0 : o1v);
      float least = qv[0] < qv[1] ? qv[0] : qv[1];
      least = qv[2] < least ? qv[2] : least;
      if (valid) {
        lo = least < lo ? least : lo;
        hi = best > hi ? best : hi;
        gap = d < gap ? d : gap;
        n_g0 += act == 0;
        n_g1 += act == 1;
        n_g2 += act == 2;
      }
      uint32_t old = 0;
      if constexpr (CMP) {
        // dword form: the four lanes of a group read the dword that the group's first lane may overwrite
        // below (remark), each its own byte of it, before that store in program order
        const size_t i = row + gr;
        if (dword) old = (*reinterpret_cast<const uint32_t*>(p.snap + (i & ~(size_t)3)) >> (8 * (i & 3))) & 0xFFu;
        else old = p.snap[i];
        n_chg += valid && old != act;
      }
      if (p.policy) store_bytes(p.policy, row + gu, valid, act, dword);
      if (p.q && valid) {
        float* qo = p.q + (row + gu) * 3;
        qo[0] = qv[0];
        qo[1] = qv[1];
        qo[2] = qv[2];
      }
      if constexpr (CMP) {
        if (p.remark) store_bytes(p.snap, row + gu, valid, act, dword);
      }
    }
    // wave 0 reads qpart before it reaches the next pass's first barrier; the others write it after
  }

  if (p.part && w == 0) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const float l2 = __shfl_xor(lo, m), h2 = __shfl_xor(hi, m), g2 = __shfl_xor(gap, m);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
      gap = g2 < gap ? g2 : gap;
      n_g0 += __shfl_xor(n_g0, m);
      n_g1 += __shfl_xor(n_g1, m);
      n_g2 += __shfl_xor(n_g2, m);
      n_chg += __shfl_xor(n_chg, m);
    }
    if (l == 0) p.part[blockIdx.x] = DqnMapPart{lo, hi, gap, {n_g0, n_g1, n_g2}, n_chg, 0u};
  }
}

// one wave per network: lanes stride over the network's bpn block partials, then fold across the wave
__global__ __launch_bounds__(kWave) void dqn_map_fold_kernel(const DqnMapParams p) {
  const size_t net = blockIdx.x;
  float lo = __builtin_inff(), hi = -__builtin_inff(), gap = __builtin_inff();
  long long c[4] = {0, 0, 0, 0};
  for (unsigned b = threadIdx.x; b < p.bpn; b += kWave) {
    const DqnMapPart x = p.part[net * p.bpn + b];
    lo = x.lo < lo ? x.lo : lo;
    hi = x.hi > hi ? x.hi : hi;
    gap = x.gap < gap ? x.gap : gap;
    c[0] += x.n_g[0];
    c[1] += x.n_g[1];
    c[2] += x.n_g[2];
    c[3] += x.n_chg;
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    const float l2 = __shfl_xor(lo, m), h2 = __shfl_xor(hi, m), g2 = __shfl_xor(gap, m);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
    gap = g2 < gap ? g2 : gap;
#pragma unroll
    for (int k = 0; k < 4; ++k) c[k] += __shfl_xor(c[k], m);
  }
  if (threadIdx.x == 0) {
    const double dlo = (double)lo, dhi = (double)hi, nlo = -dlo;
    if (p.stat_out) {
      double* out = p.stat_out + net * kDqnMapStats;
      // x + 0.0 returns a zero as +0.0 whichever of -0.0 / +0.0 the scan met first
      out[0] = (double)(c[0] + c[1] + c[2]);
      out[1] = dlo + 0.0;
      out[2] = dhi + 0.0;
      out[3] = (nlo > dhi ? nlo : dhi) + 0.0;
      out[4] = (double)c[0];
      out[5] = (double)c[1];
      out[6] = (double)c[2];
      out[7] = (double)gap + 0.0;
    }
    if (p.chg_out) p.chg_out[net] = c[3];
  }
}

}  // namespace

unsigned dqn_map_blocks(int count, uint32_t g_count) {
  if (count <= 0 || g_count == 0) return 1;
  const unsigned passes = (g_count + kPass - 1) / kPass;
  const unsigned want = (kResident + (unsigned)count - 1) / (unsigned)count;
  return passes < want ? passes : want;
}

hipError_t launch_dqn_map(const DqnMapParams& p, hipStream_t stream) {
  if (p.count <= 0 || p.g_count == 0) return hipSuccess;
  const uint64_t G = (uint64_t)p.n[0] * p.n[1] * p.n[2] * p.n[3];
  if (!p.theta || !p.axes || p.bpn == 0 || !p.n[0] || !p.n[1] || !p.n[2] || !p.n[3] || G > 0x7FFFFFFFull ||
      (uint64_t)p.g_begin + p.g_count > G || (!p.policy && !p.q && !p.part) || (p.part && !p.stat_out && !p.chg_out) ||
      (p.snap && (!p.part || !p.chg_out)) || (p.dword && p.g_count % 4 != 0) ||
      (uint64_t)p.count * p.bpn > 0x7FFFFFFFull)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)p.count * p.bpn), b(kBlock);
  if (p.snap) hipLaunchKernelGGL((dqn_map_kernel<true>), g, b, 0, stream, p);
  else hipLaunchKernelGGL((dqn_map_kernel<false>), g, b, 0, stream, p);
  if (p.part) hipLaunchKernelGGL(dqn_map_fold_kernel, dim3((unsigned)p.count), dim3(kWave), 0, stream, p);
  return hipGetLastError();
}

}  // namespace p2pmg
