// p2pmg_dqn_ops.h — the MFMA, DPP and permlane helpers that define the summation order of the DQN
// kernels (p2pmg_dqn_act.hip, p2pmg_dqn_act_shared.hip, p2pmg_dqn_train.hip, p2pmg_dqn_shared.hip: act,
// train, forward; p2pmg_dqn_eval.hip: the one-launch greedy episode; p2pmg_dqn_map.hip: the policy map).  One copy: the order of a
// reduction below is part of the bit-for-bit contract with oracle/dqn.py (fmaf chain in k order for the
// f32 MFMA, the pairwise tree of tree_sum for the lane sums).  Included inside the including unit's
// anonymous namespace, after p2pmg_device.h.
constexpr int kH = 64;
constexpr int kLdsRow = 68;  // padded activation rows: an MFMA A-operand read (16 rows x 4 k) hits 64 banks

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float relu(float x) { return x > 0.0f ? x : 0.0f; }

// Cross-lane sums as VALU lane moves (DPP and gfx950's v_permlane16/32_swap) instead of
// ds_bpermute round trips through the LDS unit.  x + swap(x) adds the same two operands in both
// lanes of every exchanged pair, so each sum below ends bitwise-identical in all its lanes.
template <int CTRL>
__device__ __forceinline__ float plus_dpp(float v) {  // v + v[lane per the DPP pattern]
  return v + __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float plus_swap16(float v) {  // rows 0 <-> 1, 2 <-> 3 (lane ^ 16)
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float plus_swap32(float v) {  // halves 0 <-> 1 (lane ^ 32)
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// over the 16 lanes of a row group: lane ^ 1, lane ^ 2 (quad_perm), the other quad of each 8
// (row_half_mirror), the other 8 of each 16 (row_mirror)
__device__ __forceinline__ float sum16(float v) {
  v = plus_dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v = plus_dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v = plus_dpp<0x141>(v);  // row_half_mirror
  v = plus_dpp<0x140>(v);  // row_mirror
  return v;
}
__device__ __forceinline__ float sum_groups(float v) {  // over the 4 row groups (same lane & 15)
  return plus_swap32(plus_swap16(v));
}
__device__ __forceinline__ float wave_sum(float v) { return sum_groups(sum16(v)); }
// sum over the 4 row groups of four values at once: the first swaps pair row groups (g4, g4 ^ 1)
// of (a, b) and of (c, d), the second (g4, g4 ^ 2) of the two pair sums, so each row group ends
// holding ONE tile's total ((g0 + g1) + (g2 + g3), sum_groups' tree); reduce4_tag() says which
// (the same swaps applied to the tile numbers)
__device__ __forceinline__ float reduce4_groups(float a, float b, float c, float d) {
  const auto r1 = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
  const auto r2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(c), __float_as_uint(d), false, false);
  const float ab = __uint_as_float(r1[0]) + __uint_as_float(r1[1]);
  const float cd = __uint_as_float(r2[0]) + __uint_as_float(r2[1]);
  const auto r3 = __builtin_amdgcn_permlane32_swap(__float_as_uint(ab), __float_as_uint(cd), false, false);
  return __uint_as_float(r3[0]) + __uint_as_float(r3[1]);
}
__device__ __forceinline__ int reduce4_tag() {
  const auto r1 = __builtin_amdgcn_permlane16_swap(0u, 1u, false, false);
  const auto r2 = __builtin_amdgcn_permlane16_swap(2u, 3u, false, false);
  const auto r3 = __builtin_amdgcn_permlane32_swap(r1[0], r2[0], false, false);
  return (int)r3[0];
}

__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
