// fgmm_like.hip — the entropy model's forward(): the differentiable likelihood of a latent under its 4-component Gaussian mixture, its
// rate and its gradients (include/flashgmm_amd.h section 3g), for CDNA4 / gfx950 (MI355X), wave64.
//
//   like_kernel       (y, sigma, mu, pi) -> the bounded likelihood per latent (optional map), v (optional), the item's bit count
//   like_bwd_kernel   (y | v, sigma, mu, pi, g | g_bits) -> dy (optional) and the twelve float32 gradient planes
//
// Each has a LOGITS form (section 3h): the weights planes hold the parameter head's logits, pi = softmax4 over K is the frame's
// (EncPlanes::get, fgmm_math.h - the sequence the coder kernels run), section 3g then runs unchanged on that pi, and the backward
// kernel stores the gradient with respect to the logits where the plain form stores dweights.  The form is a template parameter: the
// plain instantiations are the code they were (profiles/likelihood_logits.md).
//
// Both run the encode frame (fgmm_encframe.h): placement in either grid, VEC-wide loads of float32 / float16 / bfloat16 planes widened
// exactly as they arrive, wave_sum64 / add64.  The EncDesc has no chan_list: every channel is evaluated, there is no census.  What torch
// eager does with about ten element-wise kernels per component - each reading and writing an [B, M, h, w] temporary that autograd keeps
// for the backward pass - is 52 B in and 4 B out per latent here (0 out for the rate alone), and the backward kernel recomputes
// everything from the inputs: 56 B in, 52 B out, nothing saved in between.
//
// The arithmetic is section 3g's, literally: binary32, no contraction (-ffp-contract=off), correctly rounded '/'; erfcf, expf and the
// binary64 log2 are the device library's.  The rate is summed in 64-bit integers - across the wave by shuffles, then one atomic per
// wave into the item's word: integer sums do not depend on the order the atomics arrive in, every run gives the same bits.
#include <hip/hip_runtime.h>

#include "fgmm_encframe.h"

namespace fgmm {

constexpr float kLikeLn2 = 0x1.62e430p-1f;

// (like_term and like_phi, a component's p_k and the density at an edge, are the frame's: fgmm_encframe.h - centroid_kernel sums them too)
__device__ __forceinline__ float like_bound(float L, float lb) { return lb > 0.0f ? max_nan(L, lb) : L; }
__device__ __forceinline__ bool like_counts(float out) { return out > 0.0f && out < INFINITY; } // (false for NaN)

template <int VEC, typename PT, bool LINEAR, bool LOGITS>
__global__ __launch_bounds__(kBlock) void like_kernel(const EncDesc *__restrict__ descs, const LikeDesc *__restrict__ ldescs, int round, float sb,
                                                      float lb) {
  const EncDesc &d = descs[blockIdx.z];
  const LikeDesc &r = ldescs[blockIdx.z];
  const int64_t hw = d.hw;
  int c;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, d.M, c, p0, active)) return;
  unsigned long long bits = 0, left_out = 0; // the lane's latents: |term| < 2^40, so a wave's sum is far from wrapping
  if (active) {
    float v[VEC], out[VEC];
    enc_load_y<VEC>(d, c, p0, v);
    EncPlanes<PT, VEC> P;
    P.load(d, c, p0);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
      P.get(e, LOGITS, mu, sg, pi);
      if (round) v[e] = __builtin_rintf(v[e]); // round-half-even == torch.round
      float L = 0.0f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float s, xu, xl;
        const float p = like_term(v[e], mu[k], sg[k], sb, s, xu, xl);
        L = L + p * pi[k];
      }
      out[e] = like_bound(L, lb);
      if (like_counts(out[e])) bits += (unsigned long long)llrint(-log2((double)out[e]) * 0x1p32);
      else ++left_out;
      if constexpr (VEC == 1) break; // (one position: no loop, see EncPlanes<PT, 1>)
    }
    if (r.like_out) enc_st<float, VEC>(r.like_out + (int64_t)c * hw + p0, out);
    if (r.v_out) enc_st<float, VEC>(r.v_out + (int64_t)c * hw + p0, v);
  }
  bits = wave_sum64(bits);
  left_out = wave_sum64(left_out);
  if ((threadIdx.x & 63) == 0) {
    if (bits) add64(r.sums, bits);
    if (left_out) add64(r.sums + 1, left_out);
  }
}

template <int VEC, typename PT, bool LINEAR, bool LOGITS>
__global__ __launch_bounds__(kBlock) void like_bwd_kernel(const EncDesc *__restrict__ descs, const LikeGradDesc *__restrict__ gdescs, int round,
                                                          float sb, float lb) {
  const EncDesc &d = descs[blockIdx.z];
  const LikeGradDesc &r = gdescs[blockIdx.z];
  const int64_t hw = d.hw;
  int c;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, d.M, c, p0, active)) return;
  if (!active) return; // (no wave reduction here)
  float v[VEC], g[VEC];
  enc_load_y<VEC>(d, c, p0, v);
  if (r.g_like) enc_ld<float, VEC>(r.g_like + (int64_t)c * hw + p0, g);
  EncPlanes<PT, VEC> P;
  P.load(d, c, p0);
  const float gb = r.g_bits;
  float ds[4][VEC], dm[4][VEC], dw[4][VEC], dy[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) {
    float mu[4], sg[4], pi[4];
    P.get(e, LOGITS, mu, sg, pi);
    const float ve = round ? __builtin_rintf(v[e]) : v[e];
    float p[4], da[4], ga[4];
    float L = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float s, xu, xl;
      p[k] = like_term(ve, mu[k], sg[k], sb, s, xu, xl);
      L = L + p[k] * pi[k];
      const float fu = like_phi(xu), fl = like_phi(xl);
      da[k] = -pi[k] * (fu - fl) / s;
      ga[k] = -pi[k] * (fu * xu - fl * xl) / s;
    }
    float ge;
    if (r.g_like) {
      ge = g[e];
    } else { // the gradient of the item's bit count: a latent that is left out of the sum has none
      const float out = like_bound(L, lb);
      ge = like_counts(out) ? -gb / (out * kLikeLn2) : 0.0f;
    }
    const float gL = (L >= lb || ge < 0.0f || lb <= 0.0f) ? ge : 0.0f; // bound_ops.py:40-42
    float dv = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dw[k][e] = gL * p[k];
      const float sgn = (float)((ve > mu[k]) - (ve < mu[k])); // torch's abs: 0 at 0
      dm[k][e] = -gL * da[k] * sgn;
      dv = dv + gL * da[k] * sgn;
      const float G = gL * ga[k];
      ds[k][e] = (sg[k] >= sb || G < 0.0f) ? G : 0.0f;
    }
    if constexpr (LOGITS) { // section 3h: dl_k = pi_k * (dpi_k - sum_j pi_j * dpi_j), the sum k ascending, on the dpi_k just formed
      const float t = ((pi[0] * dw[0][e] + pi[1] * dw[1][e]) + pi[2] * dw[2][e]) + pi[3] * dw[3][e];
#pragma unroll
      for (int k = 0; k < 4; ++k) dw[k][e] = pi[k] * (dw[k][e] - t);
    }
    dy[e] = round ? 0.0f : dv;
    if constexpr (VEC == 1) break;
  }
  const int64_t at = (int64_t)c * hw + p0, plane = (int64_t)d.M * hw;
  if (r.dy) enc_st<float, VEC>(r.dy + at, dy);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (r.dscales) enc_st<float, VEC>(r.dscales + k * plane + at, ds[k]);
    if (r.dmeans) enc_st<float, VEC>(r.dmeans + k * plane + at, dm[k]);
    if (r.dweights) enc_st<float, VEC>(r.dweights + k * plane + at, dw[k]);
  }
}

// ---------------------------------------------------------------------------------------------------------
// launchers: a ladder over VEC (1, 4, and 8 for two-byte planes where the kernel has it) x plane type x grid
// ---------------------------------------------------------------------------------------------------------
template <bool LOGITS> struct LikeLaunch {
  const EncDesc *d;
  const LikeDesc *r;
  int round;
  float sb, lb;
  static constexpr bool kVec8 = true;
  template <int VEC, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    hipLaunchKernelGGL((like_kernel<VEC, PT, LINEAR, LOGITS>), grid, dim3(kBlock), 0, s, d, r, round, sb, lb);
  }
};
template <bool LOGITS> struct LikeBwdLaunch {
  const EncDesc *d;
  const LikeGradDesc *r;
  int round;
  float sb, lb;
  static constexpr bool kVec8 = false; // twelve VEC-wide gradient planes per lane: 4 positions keep the kernel out of scratch
  template <int VEC, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    hipLaunchKernelGGL((like_bwd_kernel<VEC, PT, LINEAR, LOGITS>), grid, dim3(kBlock), 0, s, d, r, round, sb, lb);
  }
};
// (the ladder itself, like_launch, is the frame's: fgmm_encframe.h - centroid_kernel's launcher runs it too)

int launch_like(const EncDesc *d_descs, const LikeDesc *d_ldescs, int round, float scale_bound, float likelihood_bound, int count, int M_max,
                int64_t hw_max, int64_t n_max, bool linear, int vec, int planes, bool logits, void *stream) {
  if (logits) return like_launch(LikeLaunch<true>{d_descs, d_ldescs, round, scale_bound, likelihood_bound}, count, M_max, hw_max, n_max, linear, vec, planes, stream);
  return like_launch(LikeLaunch<false>{d_descs, d_ldescs, round, scale_bound, likelihood_bound}, count, M_max, hw_max, n_max, linear, vec, planes, stream);
}
int launch_like_bwd(const EncDesc *d_descs, const LikeGradDesc *d_gdescs, int round, float scale_bound, float likelihood_bound, int count, int M_max,
                    int64_t hw_max, int64_t n_max, bool linear, int vec, int planes, bool logits, void *stream) {
  vec = vec > 4 ? 4 : vec;
  if (logits) return like_launch(LikeBwdLaunch<true>{d_descs, d_gdescs, round, scale_bound, likelihood_bound}, count, M_max, hw_max, n_max, linear, vec, planes, stream);
  return like_launch(LikeBwdLaunch<false>{d_descs, d_gdescs, round, scale_bound, likelihood_bound}, count, M_max, hw_max, n_max, linear, vec, planes, stream);
}

} // namespace fgmm
