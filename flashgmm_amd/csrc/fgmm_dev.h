// fgmm_dev.h — device helpers shared by fgmm_kernels.hip (encode side, misc), fgmm_tab.hip (decode-side tables), fgmm_rate.hip and fgmm_rdoq.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "fgmm_internal.h"
#include "fgmm_math.h"

namespace fgmm {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------------------------------
// wave / block helpers (wave64)
// ---------------------------------------------------------------------------------------------------------
// min / max that KEEP NaN, as torch.min / torch.max do (fminf / fmaxf drop it): y.max() of a latent with one NaN is NaN, and
// abs_max is then 1 (entropy_models.py:834-837) - the channel census must carry the NaN to the host
__device__ __forceinline__ float min_nan(float a, float b) { return (a < b || a != a) ? a : b; }
__device__ __forceinline__ float max_nan(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min_nan(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max_nan(v, __shfl_xor(v, o, 64));
  return v;
}

// parameter planes are float32, or float16 converted on load (BASELINE configs[4]: "fp16 (mu,sigma,pi) with fp32 CDF
// accumulate"), or bfloat16 (its 16 bits become the upper half of the binary32 pattern: one shift or mask, NaN payloads, infinities,
// signed zeros and subnormals kept): every value is widened exactly, then the fp32 path runs unchanged
// Descriptor pointers are generic (they come out of a struct in memory): cast to the global address space so that the
// accesses are global_load / global_store (a flat_load also takes a slot of the LDS queue and is waited for out of order).
#define FGMM_GLOBAL __attribute__((address_space(1)))
#ifndef FGMM_NT_LOADS
#define FGMM_NT_LOADS 1 // stream the inputs with the non-temporal hint (measured +3-4 % on the symtab kernel; 0: A/B)
#endif
template <typename T> __device__ __forceinline__ T ldg(const void *p) {
  const FGMM_GLOBAL T *g = (const FGMM_GLOBAL T *)p;
#if FGMM_NT_LOADS
  return __builtin_nontemporal_load(g);
#else
  return *g;
#endif
}
template <typename T> __device__ __forceinline__ void stg(void *p, T v) { *(FGMM_GLOBAL T *)p = v; }
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef __bf16 bfloat4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));
template <typename PT> __device__ __forceinline__ float ld1(const void *base, int64_t idx) {
  return (float)ldg<PT>(static_cast<const PT *>(base) + idx);
}
template <typename PT> __device__ __forceinline__ void ld4(const void *base, int64_t idx, float (&out)[4]);
template <> __device__ __forceinline__ void ld4<float>(const void *base, int64_t idx, float (&out)[4]) {
  const float4_t v = ldg<float4_t>(static_cast<const float *>(base) + idx); // 16 B / lane
  out[0] = v[0]; out[1] = v[1]; out[2] = v[2]; out[3] = v[3];
}
template <> __device__ __forceinline__ void ld4<_Float16>(const void *base, int64_t idx, float (&out)[4]) {
  const half4_t v = ldg<half4_t>(static_cast<const _Float16 *>(base) + idx); // 8 B / lane
  out[0] = (float)v[0]; out[1] = (float)v[1]; out[2] = (float)v[2]; out[3] = (float)v[3];
}
template <> __device__ __forceinline__ void ld4<__bf16>(const void *base, int64_t idx, float (&out)[4]) {
  const bfloat4_t v = ldg<bfloat4_t>(static_cast<const __bf16 *>(base) + idx); // 8 B / lane
  out[0] = (float)v[0]; out[1] = (float)v[1]; out[2] = (float)v[2]; out[3] = (float)v[3];
}

// N consecutive parameters (N = 2, 4), widened to float
template <typename PT, int N> __device__ __forceinline__ void ldv(const void *base, int64_t idx, float (&out)[N]) {
  typedef PT pvec_t __attribute__((ext_vector_type(N)));
  const pvec_t v = ldg<pvec_t>(static_cast<const PT *>(base) + idx);
#pragma unroll
  for (int e = 0; e < N; ++e) out[e] = (float)v[e];
}

// One entry of the encode-side table: both CDF edges of a symbol as one packed-fp32 pair, 16-bit quantisation, pmf == 0 -> the
// reference's bypass escape (rans_interface.cpp:498-517).  Shared by symtab_kernel (parameters from planes) and the fused parameter
// head (parameters straight from the MFMA accumulators, fgmm_head.hip).
// the entry of symbol vi from its two quantised edges                                      (rans_interface.cpp:512-517)
__device__ __forceinline__ uint32_t entry_from_edges(uint32_t lo, uint32_t hi, int vi, int &bypass) {
  const uint32_t pmf = (hi - lo) & 0xFFFFu; // uint16_t pmf = next - value                (:512)
  bypass = (pmf == 0);
  return pmf ? (lo | (pmf << 16)) : ((uint32_t)vi & 0xFFFFu); // bypass: low 16 bits of the int32 symbol
}
template <int MODE, bool CLAMPED>
__device__ __forceinline__ uint32_t sym_entry(float vq, int vi, const float (&mu)[4], const float (&sg)[4], const float (&pi)[4],
                                              int &bypass) {
  const float x1 = vq - 0.5f;          // static_cast<float>(value) - offset             (:499)
  const float x2 = vq - 0.5f + 1.0f;   // static_cast<float>(value) - offset + 1.0f
  uint32_t lo, hi;
  if constexpr (CLAMPED) {
    Sigma4 S;
    S.set(sg[0], sg[1], sg[2], sg[3]); // clamp + refined reciprocals, shared by both edges
    bool ok = S.tame;
    const f2 cc = mix4_clamped2<MODE>((f2){x1, x2}, mu, S, pi, ok); // both edges share every parameter: packed fp32
    float c1 = cc.x, c2 = cc.y;
    if (__builtin_expect(!ok, 0)) { // far-off / non-finite mean, NaN sigma: one rare out-of-line IEEE evaluation
      const float s0 = clamp_scale(sg[0]), s1 = clamp_scale(sg[1]), s2 = clamp_scale(sg[2]), s3 = clamp_scale(sg[3]);
      c1 = mix4_slow<MODE>(x1, mu[0], mu[1], mu[2], mu[3], s0, s1, s2, s3, pi[0], pi[1], pi[2], pi[3]);
      c2 = mix4_slow<MODE>(x2, mu[0], mu[1], mu[2], mu[3], s0, s1, s2, s3, pi[0], pi[1], pi[2], pi[3]);
    }
    lo = quant16(c1);
    hi = quant16(c2);
  } else {
    lo = quant16(mix4<MODE>(x1, mu, sg, pi));
    hi = quant16(mix4<MODE>(x2, mu, sg, pi));
  }
  return entry_from_edges(lo, hi, vi, bypass);
}

// The quantised CDF at the FOUR edges vq - 1.5, vq - 0.5, vq + 0.5, vq + 1.5 of a latent with |vq| <= 2^20 (rdoq_kernel, fgmm_rdoq.hip):
// there every edge is exact in binary32, so q[j], q[j + 1] are the `lo`, `hi` sym_entry computes for the symbol vq - 1 + j (its
// float(v) - 0.5f and float(v) - 0.5f + 1.0f are these numbers), and entry_from_edges(q[j], q[j + 1], v) is its entry.  Clamped: two
// packed pairs that share one Sigma4; a pair outside the fast cores' domain takes the IEEE evaluation edge by edge, as sym_entry's does
// (inside the domain the two agree bit for bit, so it does not matter which pair an edge falls in).
template <int MODE, bool CLAMPED>
__device__ __forceinline__ void sym_edges4(float vq, const float (&mu)[4], const float (&sg)[4], const float (&pi)[4], uint32_t (&q)[4]) {
  const float x[4] = {vq - 1.5f, vq - 0.5f, vq + 0.5f, vq + 1.5f};
  float c[4];
  if constexpr (CLAMPED) {
    Sigma4 S;
    S.set(sg[0], sg[1], sg[2], sg[3]);
    bool ok_a = S.tame, ok_b = S.tame;
    const f2 a = mix4_clamped2<MODE>((f2){x[0], x[1]}, mu, S, pi, ok_a);
    const f2 b = mix4_clamped2<MODE>((f2){x[2], x[3]}, mu, S, pi, ok_b);
    c[0] = a.x; c[1] = a.y; c[2] = b.x; c[3] = b.y;
    if (__builtin_expect(!(ok_a && ok_b), 0)) {
      const float s0 = clamp_scale(sg[0]), s1 = clamp_scale(sg[1]), s2 = clamp_scale(sg[2]), s3 = clamp_scale(sg[3]);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!(j < 2 ? ok_a : ok_b)) c[j] = mix4_slow<MODE>(x[j], mu[0], mu[1], mu[2], mu[3], s0, s1, s2, s3, pi[0], pi[1], pi[2], pi[3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) c[j] = mix4<MODE>(x[j], mu, sg, pi);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) q[j] = quant16(c[j]);
}

// ---- exact code lengths (fgmm_rate.hip, fgmm_rdoq.hip): integer costs, summed in uint64 across the wave, one atomic per wave ----------
__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ void add64(unsigned long long *p, unsigned long long v) { // no value returned: the wave does not wait for it
  (void)__hip_atomic_fetch_add((FGMM_GLOBAL unsigned long long *)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the symbol a bypass entry codes: the raw symbol, or the rounded latent converted as the host converts it (torch's .int():
// INT32_MIN for NaN, infinities and everything beyond int32 - fgmm_encode.cpp side_info)
__device__ __forceinline__ uint32_t entry_cost(uint32_t ent, float vq, int vi, bool from_y, const uint32_t *__restrict__ L) {
  if (__builtin_expect((ent >> 16) != 0, 1)) return (16u << FGMM_RATE_Q) - L[ent >> 16];
  return rate_cost_q(0u, from_y ? cvtt_i32(vq) : vi, L);
}

__device__ __forceinline__ uint32_t block_reduce_add(uint32_t v, uint32_t *s_tmp) { // kBlock threads, result in all
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) s_tmp[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0;
#pragma unroll
  for (int i = 0; i < kBlock / 64; ++i) t += s_tmp[i];
  __syncthreads();
  return t;
}
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *s_tmp) { // exclusive prefix over the block
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_tmp[w] = incl;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < w; ++i) base += s_tmp[i];
  __syncthreads();
  return base + incl - v;
}

// the same with 64-bit sums (values that may add up past 2^32 within one block)
__device__ __forceinline__ unsigned long long block_scan_excl64(unsigned long long v, unsigned long long *s_tmp) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  if (lane == 63) s_tmp[w] = incl;
  __syncthreads();
  unsigned long long base = 0;
  for (int i = 0; i < w; ++i) base += s_tmp[i];
  __syncthreads();
  return base + incl - v;
}

} // namespace fgmm
