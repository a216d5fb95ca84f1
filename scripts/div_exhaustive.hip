// Exhaustive check of the range-free f32 division forms of p2pmg_fastmath.h against the IEEE
// quotient, over EVERY pair of 24-bit significands (2^23 x 2^23 = 7.0e13 pairs).
//
// The kernels divide a / b with a hoisted reciprocal y = fma(fma(-b, y0, 1), y0, y0), y0 =
// v_rcp_f32(b) (recip()), then Newton corrections of q0 = a * y:
//   two corrections (fdiv_core, in use):  r = fma(-b, q0, a); q1 = fma(r, y, q0);
//                                         r = fma(-b, q1, a); q  = fma(r, y, q1)
//   one correction (the candidate):       r = fma(-b, q0, a); q  = fma(r, y, q0)
// Inside the range the kernels use (|a|, |b| in [2^-40, 2^40], no denormal or overflowing
// intermediate), every step scales exactly with the operands' exponents, and round-to-nearest is
// sign-symmetric, so the significand pairs a, b in [1, 2) decide every case -- PROVIDED v_rcp_f32
// itself scales exactly: y0(b 2^e) == y0(b) 2^-e.  Pass 1 checks that for every significand and
// every e in [-40, 40]; pass 2 compares both division forms with the IEEE operator for every pair.
//
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -o div_exhaustive div_exhaustive.hip
//   ./div_exhaustive [launches=32]    # one JSON line per launch, then a summary line
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x)                                                                             \
  do {                                                                                    \
    hipError_t e_ = (x);                                                                  \
    if (e_ != hipSuccess) {                                                               \
      fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
      exit(1);                                                                            \
    }                                                                                     \
  } while (0)

constexpr uint32_t kSig = 1u << 23;       // significands per binade
constexpr int kChunksA = 64;              // numerator chunks (grid.y)
constexpr uint32_t kPerChunk = kSig / kChunksA;
constexpr int kMaxSamples = 256;

struct Out {
  unsigned long long bad1, bad2, scale_bad, bad0;  // bad0: q0 = a y uncorrected (must be > 0)
  uint32_t nsamp;
  uint32_t samples[kMaxSamples][3];  // {A, B, which}
};

__device__ __forceinline__ float recip_y(float b) {
  const float y0 = __builtin_amdgcn_rcpf(b);
  return __builtin_fmaf(__builtin_fmaf(-b, y0, 1.0f), y0, y0);
}

__device__ __forceinline__ void note(Out* o, uint32_t A, uint32_t B, uint32_t which) {
  const uint32_t k = atomicAdd(&o->nsamp, 1u);
  if (k < kMaxSamples) {
    o->samples[k][0] = A;
    o->samples[k][1] = B;
    o->samples[k][2] = which;
  }
}

// pass 1: v_rcp_f32 and the refined reciprocal scale exactly with the divisor's exponent
__global__ void scale_kernel(Out* o) {
  const uint32_t B = blockIdx.x * blockDim.x + threadIdx.x;
  if (B >= kSig) return;
  const float b = __uint_as_float(0x3F800000u | B);
  const float y0 = __builtin_amdgcn_rcpf(b), y = recip_y(b);
  unsigned long long bad = 0;
  for (int e = -40; e <= 40; ++e) {
    const float be = ldexpf(b, e);
    const float y0e = __builtin_amdgcn_rcpf(be), ye = recip_y(be);
    bad += (y0e != ldexpf(y0, -e)) + (ye != ldexpf(y, -e));
  }
  if (bad) {
    atomicAdd(&o->scale_bad, bad);
    note(o, 0, B, 3);
  }
}

// pass 2: every numerator significand A of chunk blockIdx.y against divisor B
__global__ __launch_bounds__(256) void pair_kernel(uint32_t b_first, Out* o) {
  const uint32_t B = b_first + blockIdx.x * blockDim.x + threadIdx.x;
  const float b = __uint_as_float(0x3F800000u | B);
  const float y = recip_y(b);
  uint32_t bad1 = 0, bad2 = 0, bad0 = 0;
  const uint32_t a0 = blockIdx.y * kPerChunk;
  for (uint32_t A = a0; A < a0 + kPerChunk; ++A) {
    const float a = __uint_as_float(0x3F800000u | A);
    const float ref = a / b;  // hipcc's IEEE f32 division (correctly rounded)
    const float q0 = a * y;
    const float r0 = __builtin_fmaf(-b, q0, a);
    const float q1 = __builtin_fmaf(r0, y, q0);
    const float r1 = __builtin_fmaf(-b, q1, a);
    const float q2 = __builtin_fmaf(r1, y, q1);
    const bool m1 = __float_as_uint(q1) != __float_as_uint(ref);
    const bool m2 = __float_as_uint(q2) != __float_as_uint(ref);
    bad0 += __float_as_uint(q0) != __float_as_uint(ref);  // the check is not vacuous
    if (m1 | m2) {
      if (bad1 + bad2 == 0) note(o, A, B, (m1 ? 1u : 0u) | (m2 ? 2u : 0u));  // first mismatch per thread
      bad1 += m1;
      bad2 += m2;
    }
  }
  if (bad1) atomicAdd(&o->bad1, (unsigned long long)bad1);
  if (bad2) atomicAdd(&o->bad2, (unsigned long long)bad2);
  if (bad0) atomicAdd(&o->bad0, (unsigned long long)bad0);
}

int main(int argc, char** argv) {
  const int launches = argc > 1 ? atoi(argv[1]) : 32;
  if (launches < 1 || kSig % (uint32_t)launches || (kSig / launches) % 256) {
    fprintf(stderr, "launches must divide 2^23 into multiples of 256\n");
    return 2;
  }
  Out* d;
  CK(hipMalloc(&d, sizeof(Out)));
  CK(hipMemset(d, 0, sizeof(Out)));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  scale_kernel<<<kSig / 256, 256>>>(d);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  const uint32_t per = kSig / (uint32_t)launches;
  Out h;
  double total_ms = 0;
  for (int l = 0; l < launches; ++l) {
    CK(hipEventRecord(e0));
    pair_kernel<<<dim3(per / 256, kChunksA), 256>>>(per * (uint32_t)l, d);
    CK(hipGetLastError());
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    total_ms += ms;
    CK(hipMemcpy(&h, d, sizeof(Out), hipMemcpyDeviceToHost));
    printf("{\"launch\": %d, \"b_first\": %u, \"b_count\": %u, \"ms\": %.1f, \"bad_one_correction\": %llu, "
           "\"bad_two_corrections\": %llu, \"rcp_scale_bad\": %llu}\n",
           l, per * (uint32_t)l, per, ms, h.bad1, h.bad2, h.scale_bad);
    fflush(stdout);
  }
  CK(hipMemcpy(&h, d, sizeof(Out), hipMemcpyDeviceToHost));
  printf("{\"summary\": true, \"pairs\": %llu, \"bad_one_correction\": %llu, \"bad_two_corrections\": %llu, "
         "\"bad_uncorrected_q0\": %llu, \"rcp_scale_checks\": %llu, \"rcp_scale_bad\": %llu, \"ms\": %.0f, \"samples\": [",
         (unsigned long long)kSig * kSig, h.bad1, h.bad2, h.bad0, (unsigned long long)kSig * 81ull * 2ull, h.scale_bad, total_ms);
  const uint32_t n = h.nsamp < (uint32_t)kMaxSamples ? h.nsamp : (uint32_t)kMaxSamples;
  for (uint32_t k = 0; k < n; ++k)
    printf("%s[%u, %u, %u]", k ? ", " : "", h.samples[k][0], h.samples[k][1], h.samples[k][2]);
  printf("], \"samples_total\": %u}\n", h.nsamp);
  CK(hipFree(d));
  return 0;
}
