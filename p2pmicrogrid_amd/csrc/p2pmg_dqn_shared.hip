// p2pmg_dqn_shared.hip — the shared DQN network's gradient path after the train kernel (reduce plus
// Adam, the segment fold, the post-exchange Adam step; Trainer._train / _soft_update rl.py:307-359)
// and the object API's forward.  The env step and the layouts: p2pmg_dqn_act.hip.
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {
#include "p2pmg_device.h"
#include "p2pmg_dqn_ops.h"
#include "p2pmg_dqn_step.h"

// shared network: each gradient segment's sum of its train workgroups' partials (blockIdx.y = the
// local segment).  A 1024-thread workgroup owns 64 parameters; its 16 waves each fold a contiguous
// run of the segment's partials in partial order (8 loads in flight), and wave 0 adds the 16 runs
// in run order: a fixed order that depends only on the segment's block count, so a segment gives the
// same sum on any rank and in any launch.  adam != 0 (one segment over every rank): the Adam step
// on that sum in the same launch; else the sum goes to segs[seg_first + segment] for the gather.
// ROLES (a role context, always with adam): blockIdx.y = the role.  Its d.bps partials follow the previous
// role's in d.grad, its network is row blockIdx.y of the four state arrays, the mean is over its S agents
// (d.inv_agents = 1 / S), and clip, tau and the step size are its own row's when the rows differ
// (d.hyp, d.lr_net: wave-uniform scalar loads), so one launch steps all N networks.
constexpr int kRedParams = 64, kRedSlices = 16, kRedBatch = 48;
template <bool ROLES>
__global__ __launch_bounds__(kRedParams * kRedSlices) void dqn_reduce_adam_kernel(const DqnParams d, int adam) {
  __shared__ float part[kRedSlices][kRedParams];
  const int j = threadIdx.x % kRedParams, sl = threadIdx.x / kRedParams;
  const int k = blockIdx.x * kRedParams + j;
  const int n_partials = d.bps;
  const int per = (n_partials + kRedSlices - 1) / kRedSlices;
  const int b0 = sl * per, b1 = min(n_partials, b0 + per);
  const size_t ko = (ROLES ? (size_t)blockIdx.y * kNetStride : 0) + k;  // this parameter in the state arrays
  // the Adam state of this parameter, loaded ahead of the partials (one memory round trip less)
  float m0 = 0.0f, v0 = 0.0f, w0 = 0.0f, tg0 = 0.0f;
  if (sl == 0 && adam && k < kDqnParams) {
    m0 = d.adam_m[ko];
    v0 = d.adam_v[ko];
    w0 = d.theta[ko];
    tg0 = d.target[ko];
  }
  float s = 0.0f;
  if (k < kDqnParams) {
    const float* g = d.grad + (size_t)blockIdx.y * n_partials * kNetStride + k;
    int b = b0;
    if (per <= kRedBatch) {
      // every load of the run in flight at once (one memory round trip instead of per / 8); the
      // zero padding is an exact no-op (s starts at +0 and a float sum of +0 and s is s, never -0)
      float v[kRedBatch];
#pragma unroll
      for (int u = 0; u < kRedBatch; ++u) v[u] = b + u < b1 ? g[(size_t)(b + u) * kNetStride] : 0.0f;
#pragma unroll
      for (int u = 0; u < kRedBatch; ++u) s += v[u];
      b = b1;
    }
    for (; b + 8 <= b1; b += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = g[(size_t)(b + u) * kNetStride];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; b < b1; ++b) s += g[(size_t)b * kNetStride];
  }
  part[sl][j] = s;
  __syncthreads();
  if (sl != 0 || k >= kDqnParams) return;
  float t = part[0][j];
#pragma unroll
  for (int r = 1; r < kRedSlices; ++r) t += part[r][j];
  if (!adam) {
    d.segs[(size_t)(d.seg_first + blockIdx.y) * kNetStride + k] = t;
    return;
  }
  if constexpr (ROLES) {
    const float4 hyp = d.hyp ? d.hyp[blockIdx.y] : make_float4(d.gamma, d.tau, d.tau_c, d.clip);
    const float lr = d.lr_net ? d.lr_net[blockIdx.y] : d.lr_t;
    float gk = t * d.inv_agents;  // shared_grad at the role's own clip
    if (k < kOffB1) gk = fminf(fmaxf(gk, -hyp.w), hyp.w);
    const AdamStep a = adam_step(d, m0, v0, w0, gk, lr);
    d.adam_m[ko] = a.m;
    d.adam_v[ko] = a.v;
    d.theta[ko] = a.w;
    d.target[ko] = soft_update(hyp.y, hyp.z, tg0, a.w);
    return;
  }
  const AdamStep a = adam_step(d, m0, v0, w0, shared_grad(d, k, t), d.lr_t);
  d.adam_m[k] = a.m;
  d.adam_v[k] = a.v;
  d.theta[k] = a.w;
  d.target[k] = soft_update(d, tg0, a.w);
}

// The segment fold alone (the multi-segment / multi-rank path): the same 16 runs, summed in the same
// order as dqn_reduce_adam_kernel, with SPT runs per thread, i.e. 16 / SPT waves per 64 parameters
// instead of 16.  A segment of few partials (8 segments of 64 at configs[4]: 4 per run) gives each
// wave a few loads, and the launch's wave count, not its bytes, set its duration.  The zero padding
// is exact, as in dqn_reduce_adam_kernel.
template <int SPT, int BATCH>
__global__ __launch_bounds__(kRedParams * kRedSlices / SPT) void dqn_fold_kernel(const DqnParams d) {
  __shared__ float part[kRedSlices][kRedParams];
  const int j = threadIdx.x % kRedParams, grp = threadIdx.x / kRedParams;
  const int k = blockIdx.x * kRedParams + j;
  const int n = d.bps, per = (n + kRedSlices - 1) / kRedSlices;
  if (k < kDqnParams) {
    const float* g = d.grad + (size_t)blockIdx.y * n * kNetStride + k;
    float v[SPT][BATCH];  // the first BATCH partials of each of the thread's runs, in flight together
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int b0 = (grp * SPT + q) * per, b1 = min(n, b0 + per);
#pragma unroll
      for (int u = 0; u < BATCH; ++u) v[q][u] = b0 + u < b1 ? g[(size_t)(b0 + u) * kNetStride] : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < SPT; ++q) {
      const int sl = grp * SPT + q, b0 = sl * per, b1 = min(n, b0 + per);
      float s = 0.0f;
#pragma unroll
      for (int u = 0; u < BATCH; ++u) s += v[q][u];
      for (int b = b0 + BATCH; b < b1; ++b) s += g[(size_t)b * kNetStride];
      part[sl][j] = s;
    }
  }
  __syncthreads();
  if (grp != 0 || k >= kDqnParams) return;
  float t = part[0][j];
#pragma unroll
  for (int r = 1; r < kRedSlices; ++r) t += part[r][j];
  d.segs[(size_t)(d.seg_first + blockIdx.y) * kNetStride + k] = t;
}

// shared network over several segments / ranks: the segments' sum in global segment order, the mean
// over every agent of every rank, clip, Adam, soft update (every rank computes the same values)
// Latency, not bandwidth (4609 parameters): the Adam state and every segment's value are loaded
// before the first add (one memory round trip instead of one per segment), then summed in order.
// The *_out arrays may be the inputs (in place: each thread reads and writes its own parameter only).
constexpr int kAdamSegBatch = 16;
__global__ __launch_bounds__(256) void dqn_adam_shared_kernel(const DqnParams d) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= kDqnParams) return;
  if (d.n_segs <= kAdamSegBatch) {
    (void)adam_shared_param<kAdamSegBatch>(d, k, true);
    return;
  }
  const float m0 = d.adam_m[k], v0 = d.adam_v[k], w0 = d.theta[k], tg0 = d.target[k];
  float t = d.segs[k];
  for (int g = 1; g < d.n_segs; ++g) t += d.segs[(size_t)g * kNetStride + k];
  const AdamStep a = adam_step(d, m0, v0, w0, shared_grad(d, k, t), d.lr_t);
  d.m_out[k] = a.m;
  d.v_out[k] = a.v;
  d.theta_out[k] = a.w;
  d.target_out[k] = soft_update(d, tg0, a.w);
}

// QNetwork.call on explicit rows (object API, rl.py:147-148): one thread per row
__global__ void dqn_forward_kernel(const float* __restrict__ th, int n, const float* __restrict__ x,
                                   float* __restrict__ q) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  float xi[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) xi[k] = x[(size_t)r * 5 + k];
  float h1[kH];
#pragma unroll
  for (int j = 0; j < kH; ++j) {
    float z = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) z = fmaf(xi[k], th[kOffW1 + k * kH + j], z);
    h1[j] = relu(z + th[kOffB1 + j]);
  }
  float out = 0.0f;
  for (int j = 0; j < kH; ++j) {
    float z = 0.0f;
#pragma unroll 16
    for (int k = 0; k < kH; ++k) z = fmaf(h1[k], th[kOffW2 + k * kH + j], z);
    out = fmaf(relu(z + th[kOffB2 + j]), th[kOffW3 + j], out);
  }
  q[r] = out + th[kOffB3];
}

}  // namespace

hipError_t launch_dqn_reduce_adam(const DqnParams& d, int segments, bool adam, hipStream_t st) {
  if (segments < 1 || d.bps < 1 || (adam && segments != 1)) return hipErrorInvalidValue;
  const dim3 grid((kDqnParams + kRedParams - 1) / kRedParams, segments);
  // the fold: runs of per = ceil(bps / 16) partials, the first 4 or 8 of each run loaded together.
  // fold_spt 0 (auto): 4 runs per thread while a run fits one 8-load batch; longer runs (one segment
  // per rank at world > 1: 512 partials, runs of 32) keep the reduce kernel's form, whose 1024 threads
  // each have a whole run of up to 48 loads in flight
  const int per = (d.bps + kRedSlices - 1) / kRedSlices;
  const bool b4 = per <= 4;
  const int spt = d.fold_spt ? d.fold_spt : (per <= 8 ? 4 : 1);
#define P2PMG_FOLD(SPT)                                                                                           \
  if (b4) hipLaunchKernelGGL((dqn_fold_kernel<SPT, 4>), grid, dim3(kRedParams * kRedSlices / SPT), 0, st, d);   \
  else hipLaunchKernelGGL((dqn_fold_kernel<SPT, 8>), grid, dim3(kRedParams * kRedSlices / SPT), 0, st, d);
  if (adam || spt == 1) {
    hipLaunchKernelGGL(dqn_reduce_adam_kernel<false>, grid, dim3(kRedParams * kRedSlices), 0, st, d, adam ? 1 : 0);
  } else if (spt == 2) {
    P2PMG_FOLD(2)
  } else if (spt == 8) {
    P2PMG_FOLD(8)
  } else if (spt == 16) {
    P2PMG_FOLD(16)
  } else {
    P2PMG_FOLD(4)
  }
#undef P2PMG_FOLD
  return hipGetLastError();
}

hipError_t launch_dqn_reduce_adam_roles(const DqnParams& d, hipStream_t st) {
  if (d.roles < 1 || d.bps < 1 || d.n_nets != d.roles) return hipErrorInvalidValue;
  const dim3 grid((kDqnParams + kRedParams - 1) / kRedParams, d.roles);
  hipLaunchKernelGGL(dqn_reduce_adam_kernel<true>, grid, dim3(kRedParams * kRedSlices), 0, st, d, 1);
  return hipGetLastError();
}

hipError_t launch_dqn_adam_shared(const DqnParams& d, hipStream_t st) {
  const int tpb = d.adam_tpb == 64 || d.adam_tpb == 128 ? d.adam_tpb : 256;
  hipLaunchKernelGGL(dqn_adam_shared_kernel, dim3((kDqnParams + tpb - 1) / tpb), dim3(tpb), 0, st, d);
  return hipGetLastError();
}

hipError_t launch_dqn_forward(const float* theta, int n, const float* x, float* q, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(dqn_forward_kernel, dim3((n + 127) / 128), dim3(128), 0, st, theta, n, x, q);
  return hipGetLastError();
}

}  // namespace p2pmg
