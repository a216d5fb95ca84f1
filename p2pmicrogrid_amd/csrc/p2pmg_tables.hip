// p2pmg_tables.hip — gfx950 kernels of the table digests (p2pmg_table_stats, p2pmg_greedy_policy,
// p2pmg_policy_mark, p2pmg_policy_changes): one streaming pass over the padded Q rows that are already
// on the device, so that 8 doubles per table, one byte per state or two counts per table travel to the
// host instead of the tables.  A post-pass: no episode kernel changes.
//
//   table_digest_kernel<QT, STATS, CMP>   lane = row (state), consecutive lanes consecutive rows: a wave
//                            reads 64 x 32 B (f64, two 16-B loads per lane) or 64 x 16 B (f32, one)
//                            contiguous bytes per step, kUnroll steps in flight per loop trip.  A block
//                            never spans tables: table = blockIdx / bpt, and the block strides over that
//                            table's rows by bpt tiles.  Per row: visited (any of the n_actions entries
//                            != 0), greedy action (first maximum, strict >), and from them
//                              STATS   min / max per lane; visited and per-action counts as popcounts of
//                                      wave ballots -> LDS -> one partial row per block
//                              policy  the byte (action, or 255 unvisited) of four neighbouring lanes
//                                      assembled into one dword store (byte stores only where a table's
//                                      byte offset is not a multiple of 4: n_states % 4 != 0)
//                              CMP     the same byte against the snapshot's -> changed / newly visited
//                                      ballots; `remark` stores the new byte over the one just read
//   table_fold_kernel        one wave per table folds the [bpt] block partials.
// Every result is a count, a minimum or a maximum, so none depends on the grid shape or on any order;
// zero extrema are returned as +0.0.  Padding columns (k >= n_actions) are loaded with the row and never
// used.
#include "p2pmg_internal.h"

namespace p2pmg {
namespace {

constexpr int kBlock = 256;                // threads per block: 4 waves
constexpr int kWaves = kBlock / kWave;
constexpr int kUnroll = 4;                 // rows per lane whose loads are in flight together
constexpr int kTile = kBlock * kUnroll;    // rows per block per loop trip
constexpr unsigned kTargetBlocks = 2048;   // 256 CUs x 8 resident blocks: the grid for many small tables

template <typename QT>
struct Row {
  QT v[kQPad];
};
__device__ __forceinline__ Row<double> load_row(const double* q, size_t r) {
  const double2* p = reinterpret_cast<const double2*>(q) + 2 * r;
  const double2 a = p[0], b = p[1];
  return {{a.x, a.y, b.x, b.y}};
}
__device__ __forceinline__ Row<float> load_row(const float* q, size_t r) {
  const float4 a = reinterpret_cast<const float4*>(q)[r];
  return {{a.x, a.y, a.z, a.w}};
}

// store byte b of every valid lane at dst[r]; dword: r of lane 4k is a multiple of 4 and rows
// r .. r + 3 are valid together (n_states % 4 == 0), so lane 4k stores the four bytes of lanes 4k .. 4k + 3
__device__ __forceinline__ void store_bytes(uint8_t* dst, size_t r, bool valid, uint32_t b, bool dword) {
  if (dword) {
    // within each quad: lane i takes lane i + 1's byte, then lane i + 2's half (DPP quad_perm [1,2,3,3], [2,3,2,3])
    const uint32_t w1 = b | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)b, 0xF9, 0xF, 0xF, false) << 8);
    const uint32_t w = w1 | ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)w1, 0xEE, 0xF, 0xF, false) << 16);
    if (valid && (threadIdx.x & 3u) == 0u) *reinterpret_cast<uint32_t*>(dst + r) = w;
  } else if (valid) {
    dst[r] = (uint8_t)b;
  }
}

__device__ __forceinline__ unsigned long long count(bool pred) { return (unsigned long long)__popcll(__ballot(pred)); }

template <typename QT, bool STATS, bool CMP>
__global__ __launch_bounds__(kBlock) void table_digest_kernel(const TableDigestParams p) {
  const unsigned tbl = blockIdx.x / p.bpt, blk = blockIdx.x - tbl * p.bpt;
  const size_t n = p.n_states;
  const int na = p.n_actions;
  const QT* q = reinterpret_cast<const QT*>(p.q) + (size_t)tbl * n * kQPad;
  uint8_t* pol = p.policy ? p.policy + (size_t)tbl * n : nullptr;
  uint8_t* snap = CMP ? p.snap + (size_t)tbl * n : nullptr;
  const bool dword = p.dword != 0;

  QT lo = (QT)__builtin_inff(), hi = -(QT)__builtin_inff();
  unsigned long long n_vis = 0, n_g[kQPad] = {0, 0, 0, 0}, n_chg = 0, n_new = 0;  // wave-uniform

  for (size_t r0 = (size_t)blk * kTile; r0 < n; r0 += (size_t)p.bpt * kTile) {
    Row<QT> row[kUnroll];
    uint32_t old[kUnroll];
    // rows past the table's end re-read its last row (in bounds) and count nowhere
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t r = r0 + (size_t)u * kBlock + threadIdx.x;
      const size_t rc = r < n ? r : n - 1;
      row[u] = load_row(q, rc);
      if constexpr (CMP) {
        // dword form: the four lanes of a group read the dword that the group's first lane may overwrite
        // below (remark), each its own byte of it
        if (dword) old[u] = (*reinterpret_cast<const uint32_t*>(snap + (rc & ~(size_t)3)) >> (8 * (rc & 3))) & 0xFFu;
        else old[u] = snap[rc];
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t r = r0 + (size_t)u * kBlock + threadIdx.x;
      const bool valid = r < n;
      const Row<QT>& x = row[u];
      bool nz = x.v[0] != (QT)0;
      int g = 0;
      QT best = x.v[0], least = x.v[0];
#pragma unroll
      for (int k = 1; k < kQPad; ++k) {
        const bool in = k < na;
        nz = nz || (in && x.v[k] != (QT)0);
        if (in && x.v[k] > best) {  // first maximum wins (rl.py:116)
          best = x.v[k];
          g = k;
        }
        if (in && x.v[k] < least) least = x.v[k];
      }
      const uint32_t byte = nz ? (uint32_t)g : 255u;
      if constexpr (STATS) {
        if (valid && least < lo) lo = least;
        if (valid && best > hi) hi = best;
        n_vis += count(valid && nz);
#pragma unroll
        for (int k = 0; k < kQPad; ++k) n_g[k] += count(valid && nz && g == k);
      }
      if (pol) store_bytes(pol, r, valid, byte, dword);
      if constexpr (CMP) {
        const uint32_t o = old[u];
        n_chg += count(valid && (o == 255u ? 0u : o) != (uint32_t)g);  // an unvisited row's greedy action is 0
        n_new += count(valid && o == 255u && nz);
        if (p.remark) store_bytes(snap, r, valid, byte, dword);
      }
    }
  }

  // wave -> LDS -> the block's partial row
  __shared__ double s_ext[kWaves][2];
  __shared__ unsigned long long s_cnt[kWaves][8];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if constexpr (STATS) {
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const QT l2 = __shfl_xor(lo, m), h2 = __shfl_xor(hi, m);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
    }
  }
  if (lane == 0) {
    s_ext[wave][0] = (double)lo;
    s_ext[wave][1] = (double)hi;
    s_cnt[wave][0] = n_vis;
#pragma unroll
    for (int k = 0; k < kQPad; ++k) s_cnt[wave][1 + k] = n_g[k];
    s_cnt[wave][5] = n_chg;
    s_cnt[wave][6] = n_new;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double l = s_ext[0][0], h = s_ext[0][1];
    unsigned long long c[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) c[k] = s_cnt[0][k];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      l = s_ext[w][0] < l ? s_ext[w][0] : l;
      h = s_ext[w][1] > h ? s_ext[w][1] : h;
#pragma unroll
      for (int k = 0; k < 7; ++k) c[k] += s_cnt[w][k];
    }
    if constexpr (STATS) {
      double2* out = reinterpret_cast<double2*>(p.stat_part + (size_t)blockIdx.x * kTableStats);
      out[0] = make_double2((double)c[0], l);
      out[1] = make_double2(h, 0.0);
      out[2] = make_double2((double)c[1], (double)c[2]);
      out[3] = make_double2((double)c[3], (double)c[4]);
    }
    if constexpr (CMP) {
      p.chg_part[2 * (size_t)blockIdx.x] = (long long)c[5];
      p.chg_part[2 * (size_t)blockIdx.x + 1] = (long long)c[6];
    }
  }
}

// one wave per table: lanes stride over the table's bpt block partials, then fold across the wave
template <bool STATS, bool CMP>
__global__ __launch_bounds__(kWave) void table_fold_kernel(const TableDigestParams p) {
  const size_t tbl = blockIdx.x;
  if constexpr (STATS) {
    double c[5] = {0.0, 0.0, 0.0, 0.0, 0.0};  // counts: integers below 2^53, their f64 sums are exact
    double lo = (double)__builtin_inff(), hi = -(double)__builtin_inff();
    for (unsigned b = threadIdx.x; b < p.bpt; b += kWave) {
      const double2* in = reinterpret_cast<const double2*>(p.stat_part + (tbl * p.bpt + b) * kTableStats);
      const double2 a0 = in[0], a1 = in[1], a2 = in[2], a3 = in[3];
      c[0] += a0.x;
      lo = a0.y < lo ? a0.y : lo;
      hi = a1.x > hi ? a1.x : hi;
      c[1] += a2.x;
      c[2] += a2.y;
      c[3] += a3.x;
      c[4] += a3.y;
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      const double l2 = __shfl_xor(lo, m), h2 = __shfl_xor(hi, m);
      lo = l2 < lo ? l2 : lo;
      hi = h2 > hi ? h2 : hi;
#pragma unroll
      for (int k = 0; k < 5; ++k) c[k] += __shfl_xor(c[k], m);
    }
    if (threadIdx.x == 0) {
      const double nlo = -lo;
      double2* out = reinterpret_cast<double2*>(p.stat_out + tbl * kTableStats);
      // x + 0.0 returns a zero extremum as +0.0 whichever of -0.0 / +0.0 the scan met first
      out[0] = make_double2(c[0], lo + 0.0);
      out[1] = make_double2(hi + 0.0, (nlo > hi ? nlo : hi) + 0.0);
      out[2] = make_double2(c[1], c[2]);
      out[3] = make_double2(c[3], c[4]);
    }
  }
  if constexpr (CMP) {
    long long chg = 0, nw = 0;
    for (unsigned b = threadIdx.x; b < p.bpt; b += kWave) {
      chg += p.chg_part[2 * (tbl * p.bpt + b)];
      nw += p.chg_part[2 * (tbl * p.bpt + b) + 1];
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {
      chg += __shfl_xor(chg, m);
      nw += __shfl_xor(nw, m);
    }
    if (threadIdx.x == 0) {
      p.chg_out[2 * tbl] = chg;
      p.chg_out[2 * tbl + 1] = nw;
    }
  }
}

template <typename QT>
void launch_typed(const TableDigestParams& p, hipStream_t stream) {
  const dim3 g((unsigned)p.count * p.bpt), b(kBlock);
  if (p.stat_part) {
    hipLaunchKernelGGL((table_digest_kernel<QT, true, false>), g, b, 0, stream, p);
    hipLaunchKernelGGL((table_fold_kernel<true, false>), dim3((unsigned)p.count), dim3(kWave), 0, stream, p);
  } else if (p.chg_part) {
    hipLaunchKernelGGL((table_digest_kernel<QT, false, true>), g, b, 0, stream, p);
    hipLaunchKernelGGL((table_fold_kernel<false, true>), dim3((unsigned)p.count), dim3(kWave), 0, stream, p);
  } else {
    hipLaunchKernelGGL((table_digest_kernel<QT, false, false>), g, b, 0, stream, p);
  }
}

}  // namespace

unsigned table_digest_blocks(int count, size_t n_states) {
  if (count <= 0 || n_states == 0) return 1;
  const size_t tiles = (n_states + kTile - 1) / kTile;
  const size_t want = (kTargetBlocks + (unsigned)count - 1) / (unsigned)count;
  return (unsigned)(tiles < want ? tiles : want);
}

hipError_t launch_table_digest(const TableDigestParams& p, int q_dtype, hipStream_t stream) {
  if (p.count <= 0 || p.n_states == 0) return hipSuccess;
  if (p.bpt == 0 || p.n_actions < 1 || p.n_actions > kQPad || (p.stat_part && p.chg_part) ||
      (p.stat_part && !p.stat_out) || (p.chg_part && (!p.chg_out || !p.snap)) ||
      (!p.stat_part && !p.chg_part && !p.policy) || (p.dword && p.n_states % 4 != 0) ||
      (size_t)p.count * p.bpt > 0x7FFFFFFFull)
    return hipErrorInvalidValue;
  if (q_dtype == 0) launch_typed<double>(p, stream);
  else launch_typed<float>(p, stream);
  return hipGetLastError();
}

}  // namespace p2pmg
