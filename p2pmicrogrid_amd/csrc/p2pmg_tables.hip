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
// The sparse table checkpoints (p2pmg_sparse_count, p2pmg_get_q_sparse, p2pmg_set_q_sparse) follow the
// digest below: the same loads, a count / offset / scatter triple for the export and a one-thread-per-row
// import.
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

// ---- sparse table checkpoints (p2pmg_sparse_count, p2pmg_get_q_sparse, p2pmg_set_q_sparse): the same
// streaming loads as the digest.  Block b of a table owns its rows [b * rpb, (b + 1) * rpb), rpb a multiple
// of kTile, so that the row order is (block, loop trip, u, wave, lane) and a row's place in the output
// is a sum of counts taken in that order.
//   sparse_count_kernel<QT>       stored rows of the block: popcounts of wave ballots -> LDS -> blk[block]
//   sparse_offset_kernel          one wave per table: ordered exclusive scan of the table's bpt block
//                                 counts in place, and the table's total
//   sparse_scatter_kernel<QT, D>  the count pass again; per loop trip the kUnroll x kWaves ballot counts
//                                 go through LDS (double-buffered: one barrier per trip), and a stored row
//                                 lands at base[table] + blk[block] + rows of earlier trips + counts of
//                                 the (u, wave) pairs before its own + its rank in the wave's ballot (mbcnt)
//   sparse_import_kernel<QT, S>   one thread per listed row writes one padded row
// No atomics anywhere: the output bytes do not depend on the grid.
constexpr unsigned kSparseTiles = 4;  // a block's rows: at most this many tiles

__device__ __forceinline__ bool nonzero_bits(double x) { return __double_as_longlong(x) != 0; }
__device__ __forceinline__ bool nonzero_bits(float x) { return __float_as_uint(x) != 0u; }
// -0.0 counts: storedness is a matter of bits, not of value
template <typename QT>
__device__ __forceinline__ bool row_stored(const Row<QT>& x, int na) {
  bool s = nonzero_bits(x.v[0]);
#pragma unroll
  for (int k = 1; k < kQPad; ++k) s = s || (k < na && nonzero_bits(x.v[k]));
  return s;
}

template <typename QT>
__global__ __launch_bounds__(kBlock) void sparse_count_kernel(const SparseParams p) {
  const unsigned tbl = blockIdx.x / p.bpt, blk = blockIdx.x - tbl * p.bpt;
  const size_t n = p.n_states;
  const QT* q = reinterpret_cast<const QT*>(p.q) + (size_t)tbl * n * kQPad;
  const size_t begin = (size_t)blk * p.rpb, end = begin + p.rpb < n ? begin + p.rpb : n;
  unsigned cnt = 0;  // wave-uniform
  for (size_t r0 = begin; r0 < end; r0 += kTile) {
    Row<QT> row[kUnroll];
    // rows past the table's end re-read its last row (in bounds) and count nowhere
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t r = r0 + (size_t)u * kBlock + threadIdx.x;
      row[u] = load_row(q, r < n ? r : n - 1);
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t r = r0 + (size_t)u * kBlock + threadIdx.x;
      cnt += (unsigned)__popcll(__ballot(r < n && row_stored(row[u], p.n_actions)));
    }
  }
  __shared__ unsigned s_cnt[kWaves];
  if ((threadIdx.x & (kWave - 1)) == 0) s_cnt[threadIdx.x / kWave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned c = s_cnt[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) c += s_cnt[w];
    p.blk[blockIdx.x] = c;
  }
}

__global__ __launch_bounds__(kWave) void sparse_offset_kernel(const SparseParams p) {
  uint32_t* c = p.blk + (size_t)blockIdx.x * p.bpt;
  const unsigned lane = threadIdx.x;
  unsigned run = 0;  // stored rows of the blocks before this trip's 64
  for (unsigned b0 = 0; b0 < p.bpt; b0 += kWave) {
    const unsigned b = b0 + lane;
    const unsigned v = b < p.bpt ? c[b] : 0u;
    unsigned inc = v;  // inclusive scan across the wave
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      const unsigned t = __shfl_up(inc, m);
      if (lane >= (unsigned)m) inc += t;
    }
    if (b < p.bpt) c[b] = run + inc - v;
    run += __shfl(inc, kWave - 1);
  }
  if (lane == 0) p.total[blockIdx.x] = (long long)run;
}

template <typename QT, typename D>
__global__ __launch_bounds__(kBlock) void sparse_scatter_kernel(const SparseParams p) {
  const unsigned tbl = blockIdx.x / p.bpt, blk = blockIdx.x - tbl * p.bpt;
  const size_t n = p.n_states;
  const int na = p.n_actions;
  const QT* q = reinterpret_cast<const QT*>(p.q) + (size_t)tbl * n * kQPad;
  D* vals = reinterpret_cast<D*>(p.out_vals);
  const size_t begin = (size_t)blk * p.rpb, end = begin + p.rpb < n ? begin + p.rpb : n;
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  size_t pos = (size_t)p.base[tbl] + p.blk[blockIdx.x];  // where this trip's first stored row goes
  // a trip writes half `buf`, the barrier, then reads it; the next trip uses the other half, and nobody
  // reaches the trip after that (this half again) before every wave has passed the next trip's barrier
  __shared__ unsigned s_w[2][kUnroll * kWaves];
  int buf = 0;
  for (size_t r0 = begin; r0 < end; r0 += kTile, buf ^= 1) {
    Row<QT> row[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t r = r0 + (size_t)u * kBlock + threadIdx.x;
      row[u] = load_row(q, r < n ? r : n - 1);
    }
    unsigned long long bal[kUnroll];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const size_t r = r0 + (size_t)u * kBlock + threadIdx.x;
      bal[u] = __ballot(r < n && row_stored(row[u], na));
      if (lane == 0) s_w[buf][u * kWaves + wave] = (unsigned)__popcll(bal[u]);
    }
    __syncthreads();
    unsigned acc = 0;  // stored rows of the trip before (u, wave 0)
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      unsigned mine = acc;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const unsigned c = s_w[buf][u * kWaves + w];
        if ((unsigned)w < wave) mine += c;
        acc += c;
      }
      if ((bal[u] >> lane) & 1ull) {
        const unsigned rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[u] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[u], 0u));
        const size_t at = pos + mine + rank;
        p.out_rows[at] = (int32_t)(r0 + (size_t)u * kBlock + threadIdx.x);
#pragma unroll
        for (int k = 0; k < kQPad; ++k)
          if (k < na) vals[at * (size_t)na + k] = (D)row[u].v[k];
      }
    }
    pos += acc;
  }
}

__device__ __forceinline__ void store_row(double* q, size_t r, const double (&v)[kQPad]) {
  double2* d = reinterpret_cast<double2*>(q) + 2 * r;
  d[0] = make_double2(v[0], v[1]);
  d[1] = make_double2(v[2], v[3]);
}
__device__ __forceinline__ void store_row(float* q, size_t r, const float (&v)[kQPad]) {
  reinterpret_cast<float4*>(q)[r] = make_float4(v[0], v[1], v[2], v[3]);
}

template <typename QT, typename S>
__global__ __launch_bounds__(kBlock) void sparse_import_kernel(const SparseImportParams p) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.total) return;
  int lo = 0, hi = p.count;  // base[lo] <= i < base[hi], base[count] = total
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (p.base[mid] <= i) lo = mid;
    else hi = mid;
  }
  const S* src = reinterpret_cast<const S*>(p.vals) + (size_t)i * p.n_actions;
  QT v[kQPad];
#pragma unroll
  for (int k = 0; k < kQPad; ++k) v[k] = k < p.n_actions ? (QT)src[k] : (QT)0;
  store_row(reinterpret_cast<QT*>(p.q), (size_t)lo * p.n_states + (size_t)p.rows[i], v);
}

bool sparse_params_ok(const SparseParams& p) {
  return p.bpt != 0 && p.rpb != 0 && p.rpb % kTile == 0 && (size_t)p.bpt * p.rpb >= p.n_states && p.n_actions >= 1 &&
         p.n_actions <= kQPad && p.blk && (size_t)p.count * p.bpt <= 0x7FFFFFFFull;
}

}  // namespace

void sparse_blocks(int count, size_t n_states, unsigned* bpt, unsigned* rpb) {
  const size_t tiles = n_states ? (n_states + kTile - 1) / kTile : 1;
  // whole tiles per block: one while the tables give fewer than kTargetBlocks blocks, then up to kSparseTiles
  size_t tpb = tiles * (size_t)(count > 0 ? count : 1) / kTargetBlocks;
  tpb = tpb < 1 ? 1 : (tpb > kSparseTiles ? kSparseTiles : tpb);
  *rpb = (unsigned)tpb * kTile;
  *bpt = (unsigned)((tiles + tpb - 1) / tpb);
}

hipError_t launch_sparse_count(const SparseParams& p, int q_dtype, hipStream_t stream) {
  if (p.count <= 0 || p.n_states == 0) return hipSuccess;
  if (!sparse_params_ok(p) || !p.total) return hipErrorInvalidValue;
  const dim3 g((unsigned)p.count * p.bpt), b(kBlock);
  if (q_dtype == 0) hipLaunchKernelGGL(sparse_count_kernel<double>, g, b, 0, stream, p);
  else hipLaunchKernelGGL(sparse_count_kernel<float>, g, b, 0, stream, p);
  hipLaunchKernelGGL(sparse_offset_kernel, dim3((unsigned)p.count), dim3(kWave), 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_sparse_scatter(const SparseParams& p, int q_dtype, int host_dtype, hipStream_t stream) {
  if (p.count <= 0 || p.n_states == 0) return hipSuccess;
  if (!sparse_params_ok(p) || !p.base || !p.out_rows || !p.out_vals) return hipErrorInvalidValue;
  const dim3 g((unsigned)p.count * p.bpt), b(kBlock);
  if (q_dtype == 0 && host_dtype == 0) hipLaunchKernelGGL((sparse_scatter_kernel<double, double>), g, b, 0, stream, p);
  else if (q_dtype == 0) hipLaunchKernelGGL((sparse_scatter_kernel<double, float>), g, b, 0, stream, p);
  else if (host_dtype == 0) hipLaunchKernelGGL((sparse_scatter_kernel<float, double>), g, b, 0, stream, p);
  else hipLaunchKernelGGL((sparse_scatter_kernel<float, float>), g, b, 0, stream, p);
  return hipGetLastError();
}

hipError_t launch_sparse_import(const SparseImportParams& p, int q_dtype, int host_dtype, hipStream_t stream) {
  if (p.count <= 0 || p.total <= 0) return hipSuccess;
  const long long blocks = (p.total + kBlock - 1) / kBlock;
  if (!p.q || !p.base || !p.rows || !p.vals || p.n_actions < 1 || p.n_actions > kQPad || blocks > 0x7FFFFFFFll)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)blocks), b(kBlock);
  if (q_dtype == 0 && host_dtype == 0) hipLaunchKernelGGL((sparse_import_kernel<double, double>), g, b, 0, stream, p);
  else if (q_dtype == 0) hipLaunchKernelGGL((sparse_import_kernel<double, float>), g, b, 0, stream, p);
  else if (host_dtype == 0) hipLaunchKernelGGL((sparse_import_kernel<float, double>), g, b, 0, stream, p);
  else hipLaunchKernelGGL((sparse_import_kernel<float, float>), g, b, 0, stream, p);
  return hipGetLastError();
}

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
