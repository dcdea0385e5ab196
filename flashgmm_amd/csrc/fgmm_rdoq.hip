// fgmm_rdoq.hip — rate-distortion optimised quantisation of a latent (include/flashgmm_amd.h section 3c), for CDNA4 / gfx950 (MI355X).
//
//   rdoq_kernel   (y, sigma, mu, pi, lambda) -> per latent of a coded channel the symbol among round(y) - 1, round(y), round(y) + 1
//                 that minimises (y - v)^2 + lambda * bits(v), bits being the coder's own cost of v under that latent's mixture
//
// rdoq_kernel runs the encode frame of symtab_kernel and rate_kernel (fgmm_encframe.h) and prices three symbols where rate_kernel prices
// one: the quantised CDF at the four edges v0 - 1.5 .. v0 + 1.5 (sym_edges4, fgmm_dev.h: two packed pairs sharing one Sigma4) gives
// the three table entries sym_entry would yield, each costs (16 << 24) - L[range] or the bypass escape's price of that symbol
// (rate_cost_q), and the objective is compared in binary64:
//   J(v) = d * d + lam_q * (double)cost_q(v),  d = (double)y - (double)v,  lam_q = lambda * 2^-24
// every operation a single IEEE operation (the file is built with -ffp-contract=off).  Start from v0; v0 - 1 if strictly smaller;
// then v0 + 1 if strictly smaller than the best so far: ties keep the earlier candidate, lambda = 0 returns round(y).  A latent
// that is not finite, or whose |v0| exceeds 2^20 (beyond it the edges of the neighbours are no longer the encoder's own), keeps v0.
// Sums (cost of v0, cost of the choice, latents moved) are integers: shuffles across the wave, one 64-bit atomic per wave and
// accumulator into the wave's channel, the same bits on every run.  52 B in (y + twelve planes), 4 B out per latent.
//   Section 3e: the WEIGHTED instantiation multiplies d * d by wt = (double)chan_w[c] * (double)pos_w[p] (exact), the factors read from the
// item's RdoqDesc; rdo_weights_check_kernel, below, is the domain check the frame runs beside the census.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fgmm_encframe.h"

namespace fgmm {

// one latent of a coded channel -> the chosen symbol as a float (+0.0 for zero); cb / ca: cost of round(y) / of the choice.  The pricing and
// the choice are the frame's (fgmm_encframe.h: rdoq_price, rdoq_choose), shared with rdcurve_kernel
template <int MODE, bool CLAMPED>
__device__ __forceinline__ float rdoq_one(float y, const float (&mu)[4], const float (&sg)[4], const float (&pi)[4], double lam_q, double wt,
                                          const uint32_t *__restrict__ L, uint32_t &cb, uint32_t &ca) {
  float vq;
  uint32_t cm, c0, cp;
  if (!rdoq_price<MODE, CLAMPED>(y, mu, sg, pi, L, vq, cm, c0, cp)) {
    cb = ca = c0;
    return vq + 0.0f;
  }
  double d0, d;
  const int pick = rdoq_choose(y, vq, cm, c0, cp, lam_q, wt, d0, d);
  cb = c0;
  ca = pick < 0 ? cm : pick > 0 ? cp : c0;
  const float v = pick < 0 ? vq - 1.0f : pick > 0 ? vq + 1.0f : vq;
  return v + 0.0f; // (-0.0 -> +0.0)
}

#ifndef FGMM_RDOQ_WAVES
#define FGMM_RDOQ_WAVES 4 // min waves per SIMD: 128 VGPRs - the four edges, three costs and the binary64 objective do not fit rate_kernel's 96
#endif
// WEIGHTED: the instantiation of section 3e - a template parameter, so that the unweighted calls run the code they ran before it (the
// factor is the constant 1.0 there) and the weighted one pays its loads and multiplies alone (registers: profiles/rdo_weights.md)
template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR, bool WEIGHTED>
__global__ __launch_bounds__(kBlock, FGMM_RDOQ_WAVES) void rdoq_kernel(const EncDesc *__restrict__ descs, const RdoqDesc *__restrict__ qdescs,
                                                                       const uint32_t *__restrict__ L) {
  const EncDesc &d = descs[blockIdx.z];
  const RdoqDesc &r = qdescs[blockIdx.z];
  const double lam_q = r.lam_q; // the item's: a scalar load
  const int64_t hw = d.hw;
  int rank;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, d.chan_list[d.M], rank, p0, active)) return; // (always a latent with its census: no raw form here)
  const int c = d.chan_list[rank];
  unsigned long long before = 0, after = 0; // the lane's latents (at most 4 * 52 bits each)
  int nchanged = 0;                         // the wave's, the same on every active lane (ballots)
  if (active) {
    float y[VEC], out[VEC];
    enc_load_y<VEC>(d, c, p0, y);
    EncPlanes<PT, VEC> P;
    P.load(d, c, p0);
    float cw = 1.0f, pw[VEC];
    if constexpr (WEIGHTED) {
      cw = rdo_chan_w(r.chan_w, c);
      rdo_pos_w<VEC>(r.pos_w, p0, pw);
    }
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
      P.get(e, d.logits, mu, sg, pi);
      uint32_t cb, ca;
      double wt = 1.0;
      if constexpr (WEIGHTED) wt = (double)cw * (double)pw[e]; // exact: two 24-bit significands
      out[e] = rdoq_one<MODE, CLAMPED>(y[e], mu, sg, pi, lam_q, wt, L, cb, ca);
      nchanged += __popcll(__ballot(out[e] != __builtin_rintf(y[e]) && y[e] == y[e]));
      before += cb;
      after += ca;
      if constexpr (VEC == 1) break; // (one position: no loop, see EncPlanes<PT, 1>)
    }
    enc_st<float, VEC>(r.y_out + (int64_t)c * hw + p0, out);
  }
  // lanes past the end of a channel are the wave's last ones: lane 0 is active whenever any lane is, and holds the wave's count of moves
  before = wave_sum64(before);
  after = wave_sum64(after);
  if ((threadIdx.x & 63) == 0 && before) { // (every symbol costs something: 0 = a wave wholly past the end of its channel)
    add64(r.chan_before + c, before);
    add64(r.chan_after + c, after);
    if (nchanged) add64(r.chan_changed + c, (unsigned long long)nchanged);
  }
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
struct RdoqLaunch {
  const EncDesc *d;
  const RdoqDesc *r;
  const uint32_t *L;
  bool weighted;
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    if (weighted)
      hipLaunchKernelGGL((rdoq_kernel<MODE, VEC, CLAMPED, PT, LINEAR, true>), grid, dim3(kBlock), 0, s, d, r, L);
    else
      hipLaunchKernelGGL((rdoq_kernel<MODE, VEC, CLAMPED, PT, LINEAR, false>), grid, dim3(kBlock), 0, s, d, r, L);
  }
};
int launch_rdoq(const EncDesc *d_descs, const RdoqDesc *d_qdescs, const uint32_t *d_log2, bool weighted, int count, int M_max, int64_t hw_max,
                int64_t n_max, bool linear, int mode, int vec, bool clamped, bool f16, void *stream) {
  return enc_launch<false>(RdoqLaunch{d_descs, d_qdescs, d_log2, weighted}, count, M_max, hw_max, n_max, linear, mode, vec, clamped, f16, stream);
}

// ---------------------------------------------------------------------------------------------------------
// section 3e's domain: every factor finite and in [0, FGMM_RDO_W_MAX] (-0.0 counts as 0).  grid = (strides over M + hw, item); a bad
// factor anywhere - coded channel or not - raises the item's word.  Runs in the frame's front half; the word comes back with the census
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rdo_weights_check_kernel(const EncDesc *__restrict__ descs, const RdoWDesc *__restrict__ wdescs,
                                                                   uint32_t *__restrict__ bad) {
  const RdoWDesc &w = wdescs[blockIdx.y];
  const int64_t M = descs[blockIdx.y].M, hw = descs[blockIdx.y].hw;
  bool any = false;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < M + hw; i += (int64_t)gridDim.x * kBlock) {
    const float *a = i < M ? w.chan_w : w.pos_w;
    if (!a) continue;
    const float v = a[i < M ? i : i - M];
    any = any || !(v >= 0.0f && v <= FGMM_RDO_W_MAX); // (false for NaN: bad)
  }
  if (__ballot(any) && (threadIdx.x & 63) == 0) atomicOr(bad + blockIdx.y, 1u);
}
int launch_rdo_weights_check(const EncDesc *d_descs, const RdoWDesc *d_wdescs, uint32_t *bad, int count, int M_max, int64_t hw_max, void *stream) {
  if (count <= 0 || (int64_t)M_max + hw_max <= 0) return 0;
  if (count > 65535) return (int)hipErrorInvalidValue; // grid.y
  const int64_t blocks = std::min<int64_t>(((int64_t)M_max + hw_max + kBlock - 1) / kBlock, 64);
  hipLaunchKernelGGL(rdo_weights_check_kernel, dim3((unsigned)blocks, (unsigned)count), dim3(kBlock), 0, (hipStream_t)stream, d_descs, d_wdescs, bad);
  return (int)hipGetLastError();
}

} // namespace fgmm
