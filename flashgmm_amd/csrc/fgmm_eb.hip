// fgmm_eb.hip — the entropy bottleneck's forward(): the differentiable likelihood of the hyper-latent under its factorized density, its
// rate and its gradients (include/flashgmm_amd.h section 3j), for CDNA4 / gfx950 (MI355X), wave64.
//
//   eb_kernel          (x, theta, med) -> the bounded likelihood per element (optional map), v (optional), every item's bit count
//   eb_bwd_kernel      (x | v, theta, med, g | g_bits) -> dx (optional) and one partial row of dH | db | dt | sum dv per workgroup
//   eb_finish_kernel   a channel's rows, in index order -> dtheta (the dM / df step applied once per channel), dmed
//   eb_quantile_kernel (theta, three targets) -> the channel's quantiles: chain(q) = target, bisected          (section 3k: update())
//   eb_pmf_kernel      (theta, start, length) -> the masses of a channel's integer support and its tail mass   (section 3k)
//
// A workgroup works inside ONE channel: it derives the channel's 58 values (softplus of the matrices, tanh of the factors) once, into
// LDS, where every lane reads them (one address per read), and walks FGMM_EB_SLICE of the channel's B * hw elements.  What torch eager does with
// about seventy small kernels on [C, 1, B*hw] temporaries, kept by autograd for the backward pass, is one read of x and one write per
// requested output here; the backward recomputes both chains from the inputs, nothing is saved in between.
//
// The forward's arithmetic is section 3j's, literally: binary32, no contraction (-ffp-contract=off), correctly rounded '/'; expf, log1pf,
// tanhf and the binary64 log2 are the device library's.  The backward evaluates the derivatives in binary64 (see there).  The likelihood
// is formed in the MIRRORED form - sig(-lo) - sig(-up) where lo + up > 0 - so that the upper tail is a difference of two small numbers,
// not of two numbers near 1.  The rate is summed in 64-bit integers (per
// item: a wave that spans several items splits its sum per item before the atomic); the gradients of the parameters are summed in a
// fixed order - lane, wave shuffles, the workgroup's waves through LDS, the channel's rows in index order - with no float atomic:
// arrival order would change the last bits of a training run that must reproduce.
#include <hip/hip_runtime.h>

#include "fgmm_dev.h"

namespace fgmm {

constexpr int kEbP = FGMM_EB_PARAMS;
constexpr float kEbLn2 = 0x1.62e430p-1f;
static_assert(FGMM_EB_SLICE % (kBlock * 4) == 0, "a slice is a whole number of passes of the workgroup at either load width");

// theta's order (the header's): layer 0 at 0: M[3] b[3] f[3]; layers 1 - 3 at 9 + 15 * (i - 1): M[9] b[3] f[3]; layer 4 at 54: M[3] b[1]
__device__ __forceinline__ int eb_kind(int i) { // 0: a matrix entry, 1: a bias, 2: a factor
  if (i < 9) return i / 3;
  if (i >= 54) return i < 57 ? 0 : 1;
  const int r = (i - 9) % 15;
  return r < 9 ? 0 : (r < 12 ? 1 : 2);
}
__device__ __forceinline__ float eb_sig(float a) { return 1.0f / (1.0f + expf(-a)); }
__device__ __forceinline__ float eb_uniform(float v) { // the same in every lane: one scalar register
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// the channel's derived values H | b | t, in theta's order, into LDS: every lane reads them from there, the same address in all lanes
// (held in scalar registers instead, 58 values next to a kernel's own state do not fit the scalar file)
__device__ __forceinline__ void eb_params(const float *__restrict__ theta, int c, float *s_par) {
  const int i = threadIdx.x;
  if (i < kEbP) {
    const float m = ((const FGMM_GLOBAL float *)theta)[(int64_t)c * kEbP + i];
    const int kind = eb_kind(i);
    s_par[i] = kind == 0 ? (m > 20.0f ? m : log1pf(expf(m))) : (kind == 2 ? tanhf(m) : m); // torch's softplus
  }
  __syncthreads();
}

// chain(x) of the header, P the channel's values (an LDS pointer); h[i], th[i]: layer i's outputs and the tanhf of its sums (unused here:
// the reverse pass runs on eb_chain64's)
template <class PT> __device__ __forceinline__ float eb_chain(PT P, float x, float (&h)[4][3], float (&th)[4][3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float a = P[j] * x + P[3 + j];
    th[0][j] = tanhf(a);
    h[0][j] = a + P[6 + j] * th[0][j];
  }
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const int o = 9 + 15 * (i - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float a = ((P[o + 3 * j] * h[i - 1][0] + P[o + 3 * j + 1] * h[i - 1][1]) + P[o + 3 * j + 2] * h[i - 1][2]) + P[o + 9 + j];
      th[i][j] = tanhf(a);
      h[i][j] = a + P[o + 12 + j] * th[i][j];
    }
  }
  return ((P[54] * h[3][0] + P[55] * h[3][1]) + P[56] * h[3][2]) + P[57];
}

// ---- the backward's arithmetic: binary64.  A parameter's gradient is a sum over the channel's elements of terms of both signs that cancels
// to a hundredth of their magnitude and less; in binary32 the terms' own rounding (the chain amplifies it by the logit, up to 40 and more)
// then shows in the sum's fifth digit.  The decisions - the bound's select, g from the bit count - are taken on the binary32 forward
// values, so that they are the forward call's; the derivatives are the chain's in binary64 on the same binary32 inputs.
__device__ __forceinline__ double eb_sig64(double a) { return 1.0 / (1.0 + exp(-a)); }
// tanh through the one exp: absolute error of a few 2^-53, which is what the chain needs of it (a + t * tanh(a), 1 - tanh(a)^2), and one
// transcendental's code and constants in the loop instead of two
__device__ __forceinline__ double eb_tanh64(double a) { return 1.0 - 2.0 / (exp(a + a) + 1.0); }
__device__ __forceinline__ void eb_params64(const float *__restrict__ theta, int c, double *s_par64) { // H | b | t in theta's order, in LDS
  const int i = threadIdx.x;
  if (i < kEbP) {
    const double m = (double)((const FGMM_GLOBAL float *)theta)[(int64_t)c * kEbP + i];
    const int kind = eb_kind(i);
    s_par64[i] = kind == 0 ? (m > 20.0 ? m : log1p(exp(m))) : (kind == 2 ? tanh(m) : m);
  }
}
// A lane's 59 binary64 sums live in LDS, one column per lane ([k][lane]: a wave's lanes side by side): in registers, next to a chain's
// 48 activations, they do not fit the file
#define FGMM_LDS __attribute__((address_space(3))) // (a pointer known to be LDS: ds_read / ds_write, not flat accesses)
struct EbAcc {
  FGMM_LDS volatile double *col;
  __device__ __forceinline__ void add(int k, double v) const { col[k * kBlock] = col[k * kBlock] + v; }
};
// chain(x) in binary64; h[i], th[i]: layer i's outputs and the tanh of its sums, for the reverse pass
template <class PT> __device__ __forceinline__ double eb_chain64(PT P, double x, double (&h)[4][3], double (&th)[4][3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const double a = P[j] * x + P[3 + j];
    th[0][j] = eb_tanh64(a);
    h[0][j] = a + P[6 + j] * th[0][j];
  }
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const int o = 9 + 15 * (i - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double a = ((P[o + 3 * j] * h[i - 1][0] + P[o + 3 * j + 1] * h[i - 1][1]) + P[o + 3 * j + 2] * h[i - 1][2]) + P[o + 9 + j];
      th[i][j] = eb_tanh64(a);
      h[i][j] = a + P[o + 12 + j] * th[i][j];
    }
  }
  return ((P[54] * h[3][0] + P[55] * h[3][1]) + P[56] * h[3][2]) + P[57];
}
// the chain in reverse: d is the gradient arriving at its output, x its input; acc gains dH | db | dt in theta's order; -> the gradient of x
template <class PT> __device__ __forceinline__ double eb_chain_bwd(PT P, double x, const double (&h)[4][3], const double (&th)[4][3], double d,
                                               const EbAcc &acc) {
  double dh[3];
  acc.add(57, d);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    acc.add(54 + k, d * h[3][k]);
    dh[k] = d * P[54 + k];
  }
#pragma unroll
  for (int i = 3; i >= 1; --i) {
    const int o = 9 + 15 * (i - 1);
    double da[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      da[j] = dh[j] + dh[j] * (P[o + 12 + j] * (1.0 - th[i][j] * th[i][j]));
      acc.add(o + 12 + j, dh[j] * th[i][j]);
      acc.add(o + 9 + j, da[j]);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc.add(o + 3 * j + k, da[j] * h[i - 1][k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) dh[k] = (P[o + k] * da[0] + P[o + 3 + k] * da[1]) + P[o + 6 + k] * da[2];
  }
  double da[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    da[j] = dh[j] + dh[j] * (P[6 + j] * (1.0 - th[0][j] * th[0][j]));
    acc.add(6 + j, dh[j] * th[0][j]);
    acc.add(3 + j, da[j]);
    acc.add(j, da[j] * x);
  }
  return (P[0] * da[0] + P[1] * da[1]) + P[2] * da[2];
}

// element e of channel c: its item b and its place in [B, C, hw]
__device__ __forceinline__ int64_t eb_at(const EbArgs &a, int c, int64_t e, int &b) {
  b = (int)(e / a.hw);
  return ((int64_t)b * a.C + c) * a.hw + (e - (int64_t)b * a.hw);
}
template <int VEC> __device__ __forceinline__ void eb_ld(const float *p, int64_t at, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4_t t = *(const FGMM_GLOBAL float4_t *)(p + at);
    v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
  } else {
    v[0] = ((const FGMM_GLOBAL float *)p)[at];
  }
}
template <int VEC> __device__ __forceinline__ void eb_st(float *p, int64_t at, const float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    float4_t t;
    t.x = v[0], t.y = v[1], t.z = v[2], t.w = v[3];
    *(FGMM_GLOBAL float4_t *)(p + at) = t;
  } else {
    ((FGMM_GLOBAL float *)p)[at] = v[0];
  }
}
__device__ __forceinline__ float eb_bound(float L, float lb) { return lb > 0.0f ? max_nan(L, lb) : L; }
__device__ __forceinline__ bool eb_counts(float out) { return out > 0.0f && out < INFINITY; } // (false for NaN)

// a wave's bits and counts into the words of the items its lanes are in: one pass of shuffles and one atomic per word and item present
__device__ __forceinline__ void eb_add_rate(unsigned long long *sums, bool active, int b, unsigned long long bits, unsigned long long left_out) {
  unsigned long long rem = __ballot(active);
  while (rem) { // (rem is the same in every lane)
    const int leader = __builtin_ctzll(rem);
    const int bc = __shfl(b, leader, 64);
    const bool mine = active && b == bc;
    const unsigned long long sb = wave_sum64(mine ? bits : 0ull), sl = wave_sum64(mine ? left_out : 0ull);
    if ((int)(threadIdx.x & 63) == leader) {
      if (sb) add64(sums + 2 * (int64_t)bc, sb);
      if (sl) add64(sums + 2 * (int64_t)bc + 1, sl);
    }
    rem &= ~__ballot(mine);
  }
}

template <int VEC> __global__ __launch_bounds__(kBlock) void eb_kernel(const EbArgs a) {
  __shared__ float s_par[64];
  const int c = (int)(blockIdx.x / (unsigned)a.S);
  const int64_t e0 = (int64_t)(blockIdx.x - (unsigned)c * (unsigned)a.S) * FGMM_EB_SLICE;
  eb_params(a.theta, c, s_par);
  const float *P = s_par;
  const float med = eb_uniform(((const FGMM_GLOBAL float *)a.med)[c]);
  for (int it = 0; it < FGMM_EB_SLICE / (kBlock * VEC); ++it) {
    const int64_t e = e0 + ((int64_t)it * kBlock + threadIdx.x) * VEC;
    if (e0 + (int64_t)it * kBlock * VEC >= a.n) break; // (the whole workgroup)
    const bool active = e < a.n;
    int b = 0;
    unsigned long long bits = 0, left_out = 0; // |term| < 2^40: a wave's sum is far from wrapping
    if (active) {
      const int64_t at = eb_at(a, c, e, b);
      float v[VEC], out[VEC];
      eb_ld<VEC>(a.x, at, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        if (a.mode) v[k] = __builtin_rintf(v[k] - med) + med;
        float h[4][3], th[4][3];
        const float lo = eb_chain(P, v[k] - 0.5f, h, th), up = eb_chain(P, v[k] + 0.5f, h, th);
        const bool flip = (lo + up) > 0.0f;
        const float L = eb_sig(flip ? -lo : up) - eb_sig(flip ? -up : lo);
        out[k] = eb_bound(L, a.lb);
        if (eb_counts(out[k])) bits += (unsigned long long)llrint(-log2((double)out[k]) * 0x1p32);
        else ++left_out;
      }
      if (a.like) eb_st<VEC>(a.like, at, out);
      if (a.v) eb_st<VEC>(a.v, at, v);
    }
    eb_add_rate(a.sums, active, b, bits, left_out);
  }
}

template <int VEC> __global__ __launch_bounds__(kBlock) void eb_bwd_kernel(const EbArgs a) {
  __shared__ float s_par[64];
  __shared__ double s_par64[64];
  __shared__ double s_red[kBlock / 64][kEbRow + 1];
  __shared__ double s_acc[kEbRow * kBlock]; // 118 KiB: one workgroup per CU, which the kernel's registers allow anyway
  const int c = (int)(blockIdx.x / (unsigned)a.S);
  const int s = (int)(blockIdx.x - (unsigned)c * (unsigned)a.S);
  const int64_t e0 = (int64_t)s * FGMM_EB_SLICE;
  eb_params64(a.theta, c, s_par64);
  eb_params(a.theta, c, s_par); // (its barrier covers s_par64 too)
  const FGMM_LDS volatile float *P = (const FGMM_LDS volatile float *)s_par;
  const FGMM_LDS volatile double *P64 = (const FGMM_LDS volatile double *)s_par64; // (volatile: read where they are used, not hoisted into 174 registers)
  const float med = eb_uniform(((const FGMM_GLOBAL float *)a.med)[c]);
  const EbAcc acc{(FGMM_LDS volatile double *)(s_acc + threadIdx.x)};
#pragma unroll
  for (int k = 0; k < kEbRow; ++k) acc.col[k * kBlock] = 0.0;
#pragma unroll 1
  for (int it = 0; it < FGMM_EB_SLICE / (kBlock * VEC); ++it) {
    const int64_t e = e0 + ((int64_t)it * kBlock + threadIdx.x) * VEC;
    if (e >= a.n) break; // (this lane: the reduction follows the loop)
    int b;
    const int64_t at = eb_at(a, c, e, b);
    float x[VEC], g[VEC], dx[VEC];
    eb_ld<VEC>(a.x, at, x);
    float gb = 0.0f;
    if (a.g_like) eb_ld<VEC>(a.g_like, at, g);
    else gb = ((const FGMM_GLOBAL float *)a.gbits)[b];
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const float v = a.mode ? __builtin_rintf(x[k] - med) + med : x[k];
      float gL;
      { // the forward call's L, in its arithmetic: what the select and g from the bit count are decided on
        float h[4][3], th[4][3];
        const float lo = eb_chain(P, v - 0.5f, h, th), up = eb_chain(P, v + 0.5f, h, th);
        const bool flip = (lo + up) > 0.0f;
        const float L = eb_sig(flip ? -lo : up) - eb_sig(flip ? -up : lo);
        float ge;
        if (a.g_like) {
          ge = g[k];
        } else { // the gradient of the item's bit count: an element that is left out of the sum has none
          const float out = eb_bound(L, a.lb);
          ge = eb_counts(out) ? -gb / (out * kEbLn2) : 0.0f;
        }
        gL = (L >= a.lb || ge < 0.0f || a.lb <= 0.0f) ? ge : 0.0f;
      }
      double dv = 0.0;
      { // the upper edge's chain, forward and in reverse; then the lower edge's
        double h[4][3], th[4][3];
        const double xe = (double)v + 0.5, up = eb_chain64(P64, xe, h, th);
        dv = eb_chain_bwd(P64, xe, h, th, (double)gL * (eb_sig64(up) * eb_sig64(-up)), acc);
      }
      {
        double h[4][3], th[4][3];
        const double xe = (double)v - 0.5, lo = eb_chain64(P64, xe, h, th);
        dv = dv + eb_chain_bwd(P64, xe, h, th, -(double)gL * (eb_sig64(lo) * eb_sig64(-lo)), acc);
      }
      acc.add(kEbP, dv);
      dx[k] = a.mode ? 0.0f : (float)dv;
    }
    if (a.dx) eb_st<VEC>(a.dx, at, dx);
  }
  // lane -> wave (shuffles) -> workgroup (LDS, the waves in index order) -> the workgroup's row
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < kEbRow; ++k) {
    double t = acc.col[k * kBlock];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t = t + __shfl_xor(t, o, 64);
    if (lane == 0) s_red[wave][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < kEbRow) {
    double t = s_red[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) t = t + s_red[w][threadIdx.x];
    ((FGMM_GLOBAL double *)a.rows)[((int64_t)c * a.S + s) * kEbRow + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(64) void eb_finish_kernel(const float *__restrict__ theta, const double *__restrict__ rows, float *__restrict__ dtheta,
                                                       float *__restrict__ dmed, int S, int mode) {
  const int c = blockIdx.x, i = threadIdx.x;
  if (i >= kEbRow) return;
  const double *r = rows + (int64_t)c * S * kEbRow + i;
  double t = r[0];
  for (int s = 1; s < S; ++s) t = t + r[(int64_t)s * kEbRow];
  if (i == kEbP) {
    if (dmed) dmed[c] = mode ? (float)t : 0.0f;
    return;
  }
  if (!dtheta) return;
  const double m = (double)theta[(int64_t)c * kEbP + i];
  const int kind = eb_kind(i);
  if (kind == 0) t = t * (m > 20.0 ? 1.0 : eb_sig64(m));
  if (kind == 2) {
    const double th = tanh(m);
    t = t * (1.0 - th * th);
  }
  dtheta[(int64_t)c * kEbP + i] = (float)t;
}

// ---- update() (header section 3k): the quantiles and the masses of the coding tables, on eb_params, eb_chain and eb_sig as they are --------
// One 64-lane workgroup per channel: 58 lanes derive the channel's values, lanes 0 - 2 each bisect chain(q) = targets[lane] on
// [-radius, radius].  A search sees its own channel and target only.  The start is the reference's non-strict one (a target that is not
// bracketed collapses the interval onto the bound it lies beyond); a step ends the search when the midpoint equals one of the ends in
// binary32, or after kEbSearchCap steps; a NaN anywhere among the chain values of a search makes its result NaN.
__global__ __launch_bounds__(64) void eb_quantile_kernel(const float *__restrict__ theta, const EbTargets tg, float radius, float *__restrict__ q) {
  __shared__ float s_par[64];
  const int c = blockIdx.x, lane = threadIdx.x;
  eb_params(theta, c, s_par);
  if (lane >= 3) return;
  const float *P = s_par;
  const float t = lane == 0 ? tg.t[0] : (lane == 1 ? tg.t[1] : tg.t[2]);
  float h[4][3], th[4][3];
  float lo = -radius, hi = radius;
  float f = eb_chain(P, hi, h, th);
  bool nan = __builtin_isnan(f);
  lo = t <= f ? lo : hi;
  f = eb_chain(P, lo, h, th);
  nan = nan || __builtin_isnan(f);
  hi = f <= t ? hi : lo;
#pragma unroll 1
  for (int it = 0; it < kEbSearchCap && !nan; ++it) {
    const float mid = (lo + hi) / 2.0f;
    if (mid == lo || mid == hi) break;
    f = eb_chain(P, mid, h, th);
    nan = __builtin_isnan(f);
    lo = f <= t ? mid : lo;
    hi = f >= t ? mid : hi;
  }
  ((FGMM_GLOBAL float *)q)[(int64_t)c * 3 + lane] = nan ? __builtin_nanf("") : (lo + hi) / 2.0f;
}

// One lane per entry of a channel's row of `stride` floats, nb workgroups per channel.  Entry i < length: eb_kernel's L (mode 0, no
// bound) of s = start + (float)i; entry length: the tail, both of its chains evaluated by the lane that writes it; the rest: +0.
__global__ __launch_bounds__(kBlock) void eb_pmf_kernel(const float *__restrict__ theta, const float *__restrict__ start, const int32_t *__restrict__ length,
                                                        int stride, int nb, float *__restrict__ pmf) {
  __shared__ float s_par[64];
  const int c = (int)(blockIdx.x / (unsigned)nb);
  const int i = (int)(blockIdx.x - (unsigned)c * (unsigned)nb) * kBlock + (int)threadIdx.x;
  eb_params(theta, c, s_par);
  if (i >= stride) return;
  const float *P = s_par;
  const float s0 = eb_uniform(((const FGMM_GLOBAL float *)start)[c]);
  const int len = __builtin_amdgcn_readfirstlane(((const FGMM_GLOBAL int32_t *)length)[c]);
  float out = 0.0f;
  float h[4][3], th[4][3];
  if (i < len) {
    const float v = s0 + (float)i;
    const float lo = eb_chain(P, v - 0.5f, h, th), up = eb_chain(P, v + 0.5f, h, th);
    const bool flip = (lo + up) > 0.0f;
    out = eb_sig(flip ? -lo : up) - eb_sig(flip ? -up : lo);
  } else if (i == len) {
    const float lo = eb_chain(P, s0 - 0.5f, h, th), up = eb_chain(P, (s0 + (float)(len - 1)) + 0.5f, h, th);
    out = eb_sig(lo) + eb_sig(-up);
  }
  ((FGMM_GLOBAL float *)pmf)[(int64_t)c * stride + i] = out;
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
int launch_eb_quantiles(const float *theta, int C, const EbTargets &targets, float radius, float *q_out, void *stream) {
  hipLaunchKernelGGL(eb_quantile_kernel, dim3((unsigned)C), dim3(64), 0, (hipStream_t)stream, theta, targets, radius, q_out);
  return (int)hipGetLastError();
}
int launch_eb_pmf(const float *theta, const float *start, const int32_t *length, int C, int stride, float *pmf, void *stream) {
  const int64_t nb = ((int64_t)stride + kBlock - 1) / kBlock, blocks = nb * C;
  if (C < 1 || stride < 1 || blocks > 0x7FFFFFFFll) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(eb_pmf_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, (hipStream_t)stream, theta, start, length, stride, (int)nb, pmf);
  return (int)hipGetLastError();
}

static bool eb_grid(const EbArgs &a, unsigned &blocks) {
  const int64_t g = (int64_t)a.C * a.S;
  blocks = (unsigned)g;
  return g >= 1 && g <= 0x7FFFFFFFll;
}
int launch_eb(const EbArgs &a, int vec, void *stream) {
  unsigned blocks;
  if (!eb_grid(a, blocks)) return (int)hipErrorInvalidValue;
  if (vec == 4) hipLaunchKernelGGL(eb_kernel<4>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(eb_kernel<1>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
int launch_eb_bwd(const EbArgs &a, void *stream) {
  unsigned blocks;
  if (!eb_grid(a, blocks)) return (int)hipErrorInvalidValue;
  // one element per lane and pass, whatever the forward's load width: the kernel is bound by its binary64 arithmetic, consecutive lanes
  // read consecutive floats, and four elements' chains unrolled side by side do not fit the register file
  hipLaunchKernelGGL(eb_bwd_kernel<1>, dim3(blocks), dim3(kBlock), 0, (hipStream_t)stream, a);
  return (int)hipGetLastError();
}
int launch_eb_finish(const float *theta, const double *rows, float *dtheta, float *dmed, int C, int S, int mode, void *stream) {
  hipLaunchKernelGGL(eb_finish_kernel, dim3((unsigned)C), dim3(64), 0, (hipStream_t)stream, theta, rows, dtheta, dmed, S, mode);
  return (int)hipGetLastError();
}

} // namespace fgmm
