// p2pmg_dayprof.hip — gfx950 kernels of p2pmg_day_profile: the records the last episode launch left on
// the device, reduced over SCENARIOS to one row per (group, slot = t % P, agent position) and one per
// (group, slot) for the community's net grid load.  A post-pass like p2pmg_summary.hip: no episode kernel
// changes, and only the [G][P][N] rows travel to the host.  Every entry is an int64 sum of fixed-point
// terms, a count or an f32 extremum (include/p2pmg.h), so the order of the reduction is free.
//
//   dayprof_init_kernel       sums to 0, the extrema's ordered-u32 images to +inf / -inf
//   dayprof_agent_kernel      lane = agent, so a wave's loads are contiguous in the [T][A] arrays and in
//                             the packed rows.  A workgroup owns a run of agent tiles and a slice of steps
//                             (DayProfPlan, p2pmg_dayprof.h).  A tile is a multiple of N agents, so a lane
//                             keeps its agent position i from tile to tile and sums in REGISTERS while its
//                             row (group, slot, i) stays the same: along the run at one step.  When the row
//                             changes it adds its registers to the workgroup's LDS tile (64-bit LDS adds,
//                             u32 LDS min / max on the ordered images); the tile is flushed once, one global
//                             atomic per touched entry per workgroup.  Without room for one slot of every
//                             group in LDS (many groups) the registers go to global atomics directly.
//   dayprof_community_kernel  lane = scenario: G_t, the sequential f32 sum over i (the oracle's seq_sum
//                             order, part of the definition), then a wave reduction per group present in
//                             the wave and one set of global atomics per (wave, step, group).
//   dayprof_decode_kernel     the u32 images back to f32, in place.
#include "p2pmg_dayprof.h"
#include "p2pmg_internal.h"
#include "p2pmg_records.h"  // PackedRow, Step, load_step

namespace p2pmg {
namespace {

__device__ __forceinline__ float pos(float x) { return x > 0.0f ? x : 0.0f; }
__device__ __forceinline__ float neg(float x) { return x < 0.0f ? -x : 0.0f; }

__global__ __launch_bounds__(kDayProfBlock) void dayprof_init_kernel(const DayProfParams p) {
  const size_t rows = (size_t)p.G * p.P * p.rec.N, crows = (size_t)p.G * p.P;
  const size_t stride = (size_t)gridDim.x * kDayProfBlock;
  const size_t first = (size_t)blockIdx.x * kDayProfBlock + threadIdx.x;
  for (size_t k = first; k < rows * kDayProfSums; k += stride) p.sums[k] = 0ull;
  for (size_t k = first; k < rows * kDayProfExtrema; k += stride) p.ext[k] = (k & 1) ? kDayProfOrdNegInf : kDayProfOrdPosInf;
  for (size_t k = first; k < crows * kDayProfComSums; k += stride) p.com_sums[k] = 0ull;
  for (size_t k = first; k < crows * kDayProfComExtrema; k += stride) p.com_ext[k] = (k & 1) ? kDayProfOrdNegInf : kDayProfOrdPosInf;
}

__global__ __launch_bounds__(kDayProfBlock) void dayprof_decode_kernel(const DayProfParams p) {
  const size_t n = (size_t)p.G * p.P * p.rec.N * kDayProfExtrema, cn = (size_t)p.G * p.P * kDayProfComExtrema;
  const size_t stride = (size_t)gridDim.x * kDayProfBlock;
  const size_t first = (size_t)blockIdx.x * kDayProfBlock + threadIdx.x;
  for (size_t k = first; k < n; k += stride) p.ext[k] = __float_as_uint(dayprof_unord(p.ext[k]));
  for (size_t k = first; k < cn; k += stride) p.com_ext[k] = __float_as_uint(dayprof_unord(p.com_ext[k]));
}

// what a lane holds for the row it is on
struct Acc {
  long long f[kDayProfSums];
  float mn[4], mx[4];  // T_in, grid, p2p, cost
};

__device__ __forceinline__ void reset(Acc& c) {
#pragma unroll
  for (int k = 0; k < kDayProfSums; ++k) c.f[k] = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) c.mn[k] = __builtin_inff(), c.mx[k] = -__builtin_inff();
}

__device__ __forceinline__ void accumulate(Acc& c, const Step& s, const float4 lv, const float4 th) {
  const float hp = s.act == 0u ? lv.x : (s.act == 1u ? lv.y : (s.act == 2u ? lv.z : lv.w));
  const float lo = pos(th.y - s.tin), hi = pos(s.tin - th.z);  // as the summary's field 10
  const float d = lo > hi ? lo : hi;
  c.f[0] += 1;
  c.f[1] += dayprof_fix(s.cost, kDayProfShiftMoney);
  c.f[2] += dayprof_fix(s.reward, kDayProfShiftMoney);
  c.f[3] += dayprof_fix(pos(s.grid), kDayProfShiftW);
  c.f[4] += dayprof_fix(neg(s.grid), kDayProfShiftW);
  c.f[5] += dayprof_fix(pos(s.p2p), kDayProfShiftW);
  c.f[6] += dayprof_fix(neg(s.p2p), kDayProfShiftW);
  c.f[7] += dayprof_fix(hp, kDayProfShiftW);
  c.f[8] += dayprof_fix(s.load, kDayProfShiftW);
  c.f[9] += dayprof_fix(s.pv, kDayProfShiftW);
  c.f[10] += dayprof_fix(s.tin, kDayProfShiftDeg);
  c.f[11] += dayprof_fix(d, kDayProfShiftDeg);
  c.f[12] += d > 0.0f ? 1 : 0;
  c.f[13] += s.act == 1u ? 1 : 0;
  c.f[14] += s.act == 2u ? 1 : 0;
  c.f[15] += s.grid > 0.0f ? 1 : 0;
  const float v[4] = {s.tin + 0.0f, s.grid + 0.0f, s.p2p + 0.0f, s.cost + 0.0f};  // -0.0 + 0.0 = +0.0
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c.mn[k] = v[k] < c.mn[k] ? v[k] : c.mn[k];
    c.mx[k] = v[k] > c.mx[k] ? v[k] : c.mx[k];
  }
}

// a lane's registers added to row `row` of sums / ext (the LDS tile's or the output's)
__device__ __forceinline__ void add_row(const Acc& c, unsigned long long* sums, uint32_t* ext, size_t row) {
#pragma unroll
  for (int k = 0; k < kDayProfSums; ++k) atomicAdd(sums + row * kDayProfSums + k, (unsigned long long)c.f[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    atomicMin(ext + row * kDayProfExtrema + 2 * k, dayprof_ord(c.mn[k]));
    atomicMax(ext + row * kDayProfExtrema + 2 * k + 1, dayprof_ord(c.mx[k]));
  }
}

template <bool PACKED, bool LDS>
__global__ __launch_bounds__(kDayProfBlock) void dayprof_agent_kernel(const DayProfParams p) {
  extern __shared__ unsigned long long tile[];  // LDS: [rows][16] sums, then [rows][8] u32 extrema images
  const int N = p.rec.N, tid = (int)threadIdx.x;
  const int rows = LDS ? p.G * p.tile_slots * N : 0;
  uint32_t* const text = reinterpret_cast<uint32_t*>(tile + (size_t)rows * kDayProfSums);
  if constexpr (LDS) {
    for (int k = tid; k < rows * kDayProfSums; k += kDayProfBlock) tile[k] = 0ull;
    for (int k = tid; k < rows * kDayProfExtrema; k += kDayProfBlock) text[k] = (k & 1) ? kDayProfOrdNegInf : kDayProfOrdPosInf;
    __syncthreads();
  }
  const int slice = (int)(blockIdx.x % (unsigned)p.n_slices), run = (int)(blockIdx.x / (unsigned)p.n_slices);
  const int ts0 = p.t0 + slice * p.slice_steps;
  const int ts1 = ts0 + p.slice_steps < p.t1 ? ts0 + p.slice_steps : p.t1;
  const int k0 = run * p.tiles_per_run;
  const int k1 = k0 + p.tiles_per_run < p.n_tiles ? k0 + p.tiles_per_run : p.n_tiles;
  if (tid < p.tile_agents) {
    const int i = tid % N, ds = tid / N, spt = p.tile_agents / N;  // position, scenario within the tile, scenarios per tile
    const size_t a_first = (size_t)p.s0 * N + tid, a_end = (size_t)p.s1 * N;
    const size_t slots = LDS ? (size_t)p.tile_slots : (size_t)p.P;
    Acc c;
    reset(c);
    long long key = -1;  // the row the registers belong to
    for (int t = ts0; t < ts1; ++t) {
      const size_t slot = LDS ? (size_t)dayprof_tile_slot(p.fold, p.P, t, ts0) : (size_t)(t % p.P);
      for (int k = k0; k < k1; ++k) {
        const size_t a = a_first + (size_t)k * p.tile_agents;
        if (a >= a_end) continue;  // the last tile's tail
        const int g = p.labels ? p.labels[p.s0 + k * spt + ds] : 0;
        if (g < 0) continue;
        const long long row = (long long)(((size_t)g * slots + slot) * N + i);
        if (row != key) {
          if (key >= 0) add_row(c, LDS ? tile : p.sums, LDS ? text : p.ext, (size_t)key);
          reset(c);
          key = row;
        }
        accumulate(c, load_step<PACKED>(p.rec, (size_t)t, a), p.rec.hp_lv[a], p.rec.thermal[a]);
      }
    }
    if (key >= 0) add_row(c, LDS ? tile : p.sums, LDS ? text : p.ext, (size_t)key);
  }
  if constexpr (LDS) {
    __syncthreads();
    // one atomic per touched entry per workgroup; a row nobody sampled (count 0) holds only identities
    auto out_row = [&](int row) {
      const int i = row % N, ls = (row / N) % p.tile_slots, g = row / N / p.tile_slots;
      const int slot = p.fold ? ls : (ts0 + ls) % p.P;
      return ((size_t)g * p.P + slot) * N + i;
    };
    for (int e = tid; e < rows * kDayProfSums; e += kDayProfBlock) {
      const int row = e / kDayProfSums;
      const unsigned long long v = tile[e];
      if (tile[row * kDayProfSums] == 0ull || v == 0ull) continue;
      atomicAdd(p.sums + out_row(row) * kDayProfSums + e % kDayProfSums, v);
    }
    for (int e = tid; e < rows * kDayProfExtrema; e += kDayProfBlock) {
      const int row = e / kDayProfExtrema, f = e % kDayProfExtrema;
      if (tile[row * kDayProfSums] == 0ull) continue;
      if (f & 1) atomicMax(p.ext + out_row(row) * kDayProfExtrema + f, text[e]);
      else atomicMin(p.ext + out_row(row) * kDayProfExtrema + f, text[e]);
    }
  }
}

template <bool PACKED>
__device__ __forceinline__ float grid_at(const SummaryParams& p, size_t k) {
  if constexpr (PACKED) return reinterpret_cast<const PackedRow*>(p.rec_pack)[k].grid;
  else return p.grid[k];
}

template <bool PACKED>
__global__ __launch_bounds__(kDayProfBlock) void dayprof_community_kernel(const DayProfParams p) {
  const int N = p.rec.N;
  const int slice = (int)(blockIdx.x % (unsigned)p.com_n_slices);
  const size_t sb = blockIdx.x / (unsigned)p.com_n_slices;
  const size_t s = (size_t)p.s0 + sb * kDayProfBlock + threadIdx.x;
  const int g = s < (size_t)p.s1 ? (p.labels ? p.labels[s] : 0) : -1;
  const int lane = (int)(threadIdx.x % kWave);
  const int ts0 = p.t0 + slice * p.com_slice_steps;
  const int ts1 = ts0 + p.com_slice_steps < p.t1 ? ts0 + p.com_slice_steps : p.t1;
  const unsigned long long present = __ballot(g >= 0);  // uniform over the wave, as every loop below
  for (int t = ts0; t < ts1; ++t) {
    float gt = 0.0f;
    if (g >= 0) {
      const size_t k0 = (size_t)t * (size_t)p.rec.A + s * (size_t)N;
#pragma unroll 8
      for (int i = 0; i < N; ++i) gt = gt + grid_at<PACKED>(p.rec, k0 + i);
    }
    const size_t slot = (size_t)(t % p.P);
    for (unsigned long long todo = present; todo;) {  // one round per group present in the wave
      const int lead = __ffsll(todo) - 1;
      const int g0 = __shfl(g, lead);
      const bool mine = g == g0;
      long long n = mine ? 1 : 0;
      long long imp = mine ? dayprof_fix(pos(gt), kDayProfShiftW) : 0;
      long long ex = mine ? dayprof_fix(neg(gt), kDayProfShiftW) : 0;
      long long pos_n = mine && gt > 0.0f ? 1 : 0;
      uint32_t mn = mine ? dayprof_ord(gt + 0.0f) : kDayProfOrdPosInf;
      uint32_t mx = mine ? dayprof_ord(gt + 0.0f) : kDayProfOrdNegInf;
#pragma unroll
      for (int w = kWave / 2; w >= 1; w >>= 1) {
        n += __shfl_xor(n, w);
        imp += __shfl_xor(imp, w);
        ex += __shfl_xor(ex, w);
        pos_n += __shfl_xor(pos_n, w);
        const uint32_t omn = (uint32_t)__shfl_xor((int)mn, w), omx = (uint32_t)__shfl_xor((int)mx, w);
        mn = omn < mn ? omn : mn;
        mx = omx > mx ? omx : mx;
      }
      if (lane == lead) {
        const size_t row = (size_t)g0 * p.P + slot;
        atomicAdd(p.com_sums + row * kDayProfComSums, (unsigned long long)n);
        if (imp) atomicAdd(p.com_sums + row * kDayProfComSums + 1, (unsigned long long)imp);
        if (ex) atomicAdd(p.com_sums + row * kDayProfComSums + 2, (unsigned long long)ex);
        if (pos_n) atomicAdd(p.com_sums + row * kDayProfComSums + 3, (unsigned long long)pos_n);
        atomicMin(p.com_ext + row * kDayProfComExtrema, mn);
        atomicMax(p.com_ext + row * kDayProfComExtrema + 1, mx);
      }
      todo &= ~__ballot(mine);
    }
  }
}

}  // namespace

hipError_t launch_day_profile(const DayProfParams& p0, hipStream_t stream) {
  DayProfParams p = p0;
  const size_t entries = (size_t)p.G * p.P * p.rec.N * kDayProfSums;
  const unsigned small = (unsigned)((entries + kDayProfBlock - 1) / kDayProfBlock < 2048 ? (entries + kDayProfBlock - 1) / kDayProfBlock : 2048);
  hipLaunchKernelGGL(dayprof_init_kernel, dim3(small), dim3(kDayProfBlock), 0, stream, p);
  const int steps = p.t1 - p.t0, scen = p.s1 - p.s0;
  if (steps > 0 && scen > 0) {
    const unsigned blocks = (unsigned)p.n_slices * (unsigned)((p.n_tiles + p.tiles_per_run - 1) / p.tiles_per_run);
    const size_t lds = p.lds ? p.tile_bytes : 0;
    if (p.rec.packed) {
      if (p.lds) hipLaunchKernelGGL((dayprof_agent_kernel<true, true>), dim3(blocks), dim3(kDayProfBlock), lds, stream, p);
      else hipLaunchKernelGGL((dayprof_agent_kernel<true, false>), dim3(blocks), dim3(kDayProfBlock), 0, stream, p);
    } else {
      if (p.lds) hipLaunchKernelGGL((dayprof_agent_kernel<false, true>), dim3(blocks), dim3(kDayProfBlock), lds, stream, p);
      else hipLaunchKernelGGL((dayprof_agent_kernel<false, false>), dim3(blocks), dim3(kDayProfBlock), 0, stream, p);
    }
    // the community pass: workgroups of kDayProfBlock scenarios, the steps cut so that about
    // kDayProfTargetBlocks workgroups run
    const unsigned sblocks = (unsigned)((scen + kDayProfBlock - 1) / kDayProfBlock);
    const int want = (int)((kDayProfTargetBlocks + sblocks - 1) / sblocks);
    p.com_n_slices = want < steps ? want : steps;
    p.com_slice_steps = (steps + p.com_n_slices - 1) / p.com_n_slices;
    p.com_n_slices = (steps + p.com_slice_steps - 1) / p.com_slice_steps;
    if (p.rec.packed) hipLaunchKernelGGL(dayprof_community_kernel<true>, dim3(sblocks * (unsigned)p.com_n_slices), dim3(kDayProfBlock), 0, stream, p);
    else hipLaunchKernelGGL(dayprof_community_kernel<false>, dim3(sblocks * (unsigned)p.com_n_slices), dim3(kDayProfBlock), 0, stream, p);
  }
  hipLaunchKernelGGL(dayprof_decode_kernel, dim3(small), dim3(kDayProfBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace p2pmg
