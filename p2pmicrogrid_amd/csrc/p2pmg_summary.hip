// p2pmg_summary.hip — gfx950 kernels of p2pmg_episode_summary: the records the last episode launch
// left on the device, reduced over time to 16 f64 values per agent and 16 per scenario (the totals
// behind the reference's figures, data_analysis.py:188-209, 324-420, 775-846).  A post-pass: no
// episode kernel changes, and only [A][16] + [S][16] doubles travel to the host.
//
//   summary_agent_kernel     lane = agent, so a wave's loads are contiguous in the [T][A] arrays
//                            (and in the packed 32-B rows).  The loop over t runs in chunks of
//                            kChunk steps: the next chunk's loads are issued before the current
//                            chunk is accumulated, in order, one step after the other.
//   summary_scenario_kernel  lane = scenario: the sequential sums over i of the agents' rows and the
//                            community's grid peaks max_t max(+-G_t, 0), G_t the sequential f32 sum
//                            over i of grid[t, s N + i] (the oracle's seq_sum order).
//
// Both read either layout a launch leaves: the plain arrays (general, tile, shared, role, rule and
// DQN launches) or the packed rows of episode_fast_kernel / episode_sq16_kernel, directly.
// The order of every sum is part of the interface (include/p2pmg.h): sequential over t, then over i,
// from +0.0, each term formed in f32 and widened.  max(x, 0) is x > 0 ? x : +0 throughout.
#include "p2pmg_internal.h"
#include "p2pmg_records.h"  // PackedRow, Step, load_step

namespace p2pmg {
namespace {

constexpr int kChunk = 4;  // steps whose loads are in flight while the previous kChunk accumulate

__device__ __forceinline__ float pos(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float neg(float x) { return x < 0.0f ? -x : 0.0f; }

struct Acc {
  double f[12];
  float t_min, t_max, peak_in, peak_out;
};

__device__ __forceinline__ void accumulate(Acc& c, const Step& s, const float4 lv, const float4 th) {
  const float gi = pos(s.grid), ge = neg(s.grid);
  const float hp = s.act == 0u ? lv.x : (s.act == 1u ? lv.y : (s.act == 2u ? lv.z : lv.w));
  const float power = s.grid + s.p2p;                          // what run() returns (community.py:121)
  const float self = power < 0.0f ? s.pv + power : s.pv;       // data_analysis.py:195
  const float lo = pos(th.y - s.tin), hi = pos(s.tin - th.z);  // agent.py:227-228
  const float d = lo > hi ? lo : hi;
  c.f[0] += (double)s.cost;
  c.f[1] += (double)s.reward;
  c.f[2] += (double)gi;
  c.f[3] += (double)ge;
  c.f[4] += (double)pos(s.p2p);
  c.f[5] += (double)neg(s.p2p);
  c.f[6] += (double)hp;
  c.f[7] += (double)s.load;
  c.f[8] += (double)s.pv;
  c.f[9] += (double)self;
  c.f[10] += (double)d;
  c.f[11] += d > 0.0f ? 1.0 : 0.0;
  c.t_min = s.tin < c.t_min ? s.tin : c.t_min;
  c.t_max = s.tin > c.t_max ? s.tin : c.t_max;
  c.peak_in = gi > c.peak_in ? gi : c.peak_in;
  c.peak_out = ge > c.peak_out ? ge : c.peak_out;
}

template <bool PACKED>
__global__ __launch_bounds__(kWave) void summary_agent_kernel(const SummaryParams p) {
  const size_t a = (size_t)blockIdx.x * kWave + threadIdx.x;
  if (a >= (size_t)p.A) return;
  const float4 lv = p.hp_lv[a];
  const float4 th = p.thermal[a];
  const int T = p.T;
  Acc c;
#pragma unroll
  for (int k = 0; k < 12; ++k) c.f[k] = 0.0;
  c.t_min = __builtin_inff();
  c.t_max = -__builtin_inff();
  c.peak_in = 0.0f;
  c.peak_out = 0.0f;
  // loads past the horizon re-read step T - 1 (in bounds) and are never accumulated
  auto fetch = [&](Step (&buf)[kChunk], int t0) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kChunk; ++j) buf[j] = load_step<PACKED>(p, (size_t)(t0 + j < T ? t0 + j : T - 1), a);
  };
  Step cur[kChunk], nxt[kChunk];
  fetch(cur, 0);
  for (int t0 = 0; t0 < T; t0 += kChunk) {
    if (t0 + kChunk < T) fetch(nxt, t0 + kChunk);
#pragma unroll
    for (int j = 0; j < kChunk; ++j)
      if (t0 + j < T) accumulate(c, cur[j], lv, th);
#pragma unroll
    for (int j = 0; j < kChunk; ++j) cur[j] = nxt[j];
  }
  double2* out = reinterpret_cast<double2*>(p.agent_out + a * kSummaryFields);
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = make_double2(c.f[2 * k], c.f[2 * k + 1]);
  out[6] = make_double2((double)c.t_min, (double)c.t_max);
  out[7] = make_double2((double)c.peak_in, (double)c.peak_out);
}

template <bool PACKED>
__device__ __forceinline__ float grid_at(const SummaryParams& p, size_t k) {
  if constexpr (PACKED) return reinterpret_cast<const PackedRow*>(p.rec_pack)[k].grid;
  else return p.grid[k];
}

// after summary_agent_kernel on the same stream: reads its [A][16] rows
template <bool PACKED>
__global__ __launch_bounds__(kWave) void summary_scenario_kernel(const SummaryParams p) {
  const size_t s = (size_t)blockIdx.x * kWave + threadIdx.x;
  if (s >= (size_t)p.S) return;
  const int N = p.N;
  const size_t a0 = s * (size_t)N;
  double f[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) f[k] = 0.0;
  double t_min = (double)__builtin_inff(), t_max = -(double)__builtin_inff();
  for (int i = 0; i < N; ++i) {
    const double2* row = reinterpret_cast<const double2*>(p.agent_out + (a0 + i) * kSummaryFields);
    double2 v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = row[k];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      f[2 * k] += v[k].x;
      f[2 * k + 1] += v[k].y;
    }
    t_min = v[6].x < t_min ? v[6].x : t_min;
    t_max = v[6].y > t_max ? v[6].y : t_max;
  }
  // the community's net load on the grid per step (plot_grid_load), its import and export peaks
  float peak_in = 0.0f, peak_out = 0.0f;
  for (int t = 0; t < p.T; ++t) {
    const size_t k0 = (size_t)t * (size_t)p.A + a0;
    float g = 0.0f;
#pragma unroll 8
    for (int i = 0; i < N; ++i) g = g + grid_at<PACKED>(p, k0 + i);
    const float gi = pos(g), ge = neg(g);
    peak_in = gi > peak_in ? gi : peak_in;
    peak_out = ge > peak_out ? ge : peak_out;
  }
  double2* out = reinterpret_cast<double2*>(p.scen_out + s * kSummaryFields);
#pragma unroll
  for (int k = 0; k < 6; ++k) out[k] = make_double2(f[2 * k], f[2 * k + 1]);
  out[6] = make_double2(t_min, t_max);
  out[7] = make_double2((double)peak_in, (double)peak_out);
}

}  // namespace

hipError_t launch_episode_summary(const SummaryParams& p, hipStream_t stream) {
  const unsigned ba = (unsigned)(((size_t)p.A + kWave - 1) / kWave), bs = (unsigned)(((size_t)p.S + kWave - 1) / kWave);
  if (p.packed) {
    hipLaunchKernelGGL(summary_agent_kernel<true>, dim3(ba), dim3(kWave), 0, stream, p);
    hipLaunchKernelGGL(summary_scenario_kernel<true>, dim3(bs), dim3(kWave), 0, stream, p);
  } else {
    hipLaunchKernelGGL(summary_agent_kernel<false>, dim3(ba), dim3(kWave), 0, stream, p);
    hipLaunchKernelGGL(summary_scenario_kernel<false>, dim3(bs), dim3(kWave), 0, stream, p);
  }
  return hipGetLastError();
}

}  // namespace p2pmg
