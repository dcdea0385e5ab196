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
//   rdoq_skip_kernel  section 3f: the channel decision over rdoq_kernel<..., SKIP>'s per-channel sums, the skipped planes zeroed
//   Section 3e: the WEIGHTED instantiation multiplies d * d by wt = (double)chan_w[c] * (double)pos_w[p] (exact), the factors read from the
// item's RdoqDesc; rdo_weights_check_kernel, below, is the domain check the frame runs beside the census.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fgmm_encframe.h"

namespace fgmm {

// one latent of a coded channel -> the chosen symbol as a float (+0.0 for zero); cb / ca: cost of round(y) / of the choice.  The pricing and
// the choice are the frame's (fgmm_encframe.h: rdoq_price, rdoq_choose), shared with rdcurve_kernel.  ONE text for both forms of rdoq_kernel:
// the SKIP form goes on with what `m` keeps of the decision, the plain form drops it (everything is inlined: what is not read is not computed)
struct RdoqMove {
  float vq;     // round(y)
  bool priced;  // false: not finite or |vq| > 2^20 - the latent kept round(y)
  int pick;     // -1 / 0 / +1 (0 when not priced)
  double d0, d; // the distances to round(y) and to the choice (set when priced)
};
template <int MODE, bool CLAMPED>
__device__ __forceinline__ float rdoq_one(float y, const float (&mu)[4], const float (&sg)[4], const float (&pi)[4], double lam_q, double wt,
                                          const uint32_t *__restrict__ L, uint32_t &cb, uint32_t &ca, RdoqMove &m) {
  uint32_t cm, c0, cp;
  m.pick = 0;
  m.priced = rdoq_price<MODE, CLAMPED>(y, mu, sg, pi, L, m.vq, cm, c0, cp);
  if (!m.priced) {
    cb = ca = c0;
    return m.vq + 0.0f;
  }
  m.pick = rdoq_choose(y, m.vq, cm, c0, cp, lam_q, wt, m.d0, m.d);
  cb = c0;
  ca = m.pick < 0 ? cm : m.pick > 0 ? cp : c0;
  const float v = m.pick < 0 ? m.vq - 1.0f : m.pick > 0 ? m.vq + 1.0f : m.vq;
  return v + 0.0f; // (-0.0 -> +0.0)
}

#ifndef FGMM_RDOQ_WAVES
#define FGMM_RDOQ_WAVES 4 // min waves per SIMD: 128 VGPRs - the four edges, three costs and the binary64 objective do not fit rate_kernel's 96
#endif
// WEIGHTED: the instantiation of section 3e - a template parameter, so that the unweighted calls run the code they ran before it (the
// factor is the constant 1.0 there) and the weighted one pays its loads and multiplies alone (registers: profiles/rdo_weights.md).
// SKIP: section 3f, a template parameter for the same reason (profiles/rdo_skip.md).  Beside the three sums the wave adds what the
// channel decision needs: Dk and Dz through wave_sum64, nz0, nzA and inelig by ballots, one 64-bit atomic each into the channel's words
template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR, bool WEIGHTED, bool SKIP>
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
  unsigned long long dk = 0, dz = 0;        // SKIP: the lane's terms of Dk (units of 2^-32) and Dz (2^-16)
  int nz0 = 0, nza = 0;                     // SKIP: the wave's (ballots)
  bool inel = false;
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
      RdoqMove mv;
      out[e] = rdoq_one<MODE, CLAMPED>(y[e], mu, sg, pi, lam_q, wt, L, cb, ca, mv);
      if constexpr (SKIP) { // what the channel decision sums
        if (mv.pick) dk += (unsigned long long)(long long)__builtin_rint((wt * (mv.d * mv.d - mv.d0 * mv.d0)) * 0x1p32);
        const bool big = !mv.priced || __builtin_fabsf(mv.vq) > (float)FGMM_SKIP_VMAX; // (not finite, or beyond 2^20: not priced)
        inel = inel || __ballot(big) != 0;
        nz0 += __popcll(__ballot(mv.vq != 0.0f));
        nza += __popcll(__ballot(out[e] != 0.0f));
        if (!big && mv.vq != 0.0f) dz += rdo_skip_dz(y[e], mv.vq, wt);
      }
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
  if constexpr (SKIP) {
    dk = wave_sum64(dk);
    dz = wave_sum64(dz);
  }
  if ((threadIdx.x & 63) == 0 && before) { // (every symbol costs something: 0 = a wave wholly past the end of its channel)
    add64(r.chan_before + c, before);
    add64(r.chan_after + c, after);
    if (nchanged) add64(r.chan_changed + c, (unsigned long long)nchanged);
    if constexpr (SKIP) {
      unsigned long long *s = r.chan_skip + c;
      const int64_t M = d.M;
      if (dk) add64(s + kRdoSkipDk * M, dk);
      if (dz) add64(s + kRdoSkipDz * M, dz);
      if (nz0) add64(s + kRdoSkipNz0 * M, (unsigned long long)nz0);
      if (nza) add64(s + kRdoSkipNzA * M, (unsigned long long)nza);
      if (inel) add64(s + kRdoSkipInelig * M, 1ull);
    }
  }
}

// Section 3f's channel decision, after rdoq_kernel<..., SKIP> on the same stream and on its grid.  Every wave of a coded channel reads the
// channel's sums (wave-uniform) and evaluates rdo_skip_rule - the same integers, the same binary64 sequence, the same answer everywhere -
// and, the channel skipped, stores +0.0 VEC-wide over its share of the plane.  The one lane at position 0 of the channel (lane 0 of its first wave, in both grids) writes the channel's
// final sums and flag to words of their own (kRdoSkipAfter ..: no decision reads them - overwriting the accumulators would race with
// the waves still reading) and adds them to the item's
template <int VEC, bool LINEAR>
__global__ __launch_bounds__(kBlock) void rdoq_skip_kernel(const EncDesc *__restrict__ descs, const RdoqDesc *__restrict__ qdescs) {
  const EncDesc &d = descs[blockIdx.z];
  const RdoqDesc &r = qdescs[blockIdx.z];
  const int64_t hw = d.hw;
  int rank;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, d.chan_list[d.M], rank, p0, active)) return;
  const int c = d.chan_list[rank];
  const int64_t M = d.M;
  unsigned long long *s = r.chan_skip + c;
  const unsigned long long A = r.chan_after[c], Dk = s[kRdoSkipDk * M], Dz = s[kRdoSkipDz * M], nz0 = s[kRdoSkipNz0 * M], nzA = s[kRdoSkipNzA * M];
  const bool inelig = s[kRdoSkipInelig * M] != 0 || hw > (1ll << 24);
  const bool skip = rdo_skip_rule(inelig, A, nzA, Dk, Dz, r.lam_q);
  if (!active) return;
  if (skip) {
    float zero[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) zero[e] = 0.0f;
    enc_st<float, VEC>(r.y_out + (int64_t)c * hw + p0, zero);
  }
  if (p0 == 0) { // one lane per channel
    const unsigned long long fa = skip ? 0ull : A, fc = skip ? nz0 : r.chan_changed[c], fd = skip ? Dz << 16 : Dk;
    s[kRdoSkipAfter * M] = fa;
    s[kRdoSkipChanged * M] = fc;
    s[kRdoSkipDd * M] = fd;
    s[kRdoSkipFlag * M] = skip ? 1ull : 0ull;
    if (fa) add64(r.item_sums + 0, fa);
    if (fc) add64(r.item_sums + 1, fc);
    if (fd) add64(r.item_sums + 2, fd);
    if (skip) add64(r.item_sums + 3, 1ull);
    if (!inelig) add64(r.item_sums + 4, 1ull);
  }
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
struct RdoqLaunch {
  const EncDesc *d;
  const RdoqDesc *r;
  const uint32_t *L;
  bool weighted, skip;
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR, bool WEIGHTED> void go_w(dim3 grid, hipStream_t s) const {
    if (skip)
      hipLaunchKernelGGL((rdoq_kernel<MODE, VEC, CLAMPED, PT, LINEAR, WEIGHTED, true>), grid, dim3(kBlock), 0, s, d, r, L);
    else
      hipLaunchKernelGGL((rdoq_kernel<MODE, VEC, CLAMPED, PT, LINEAR, WEIGHTED, false>), grid, dim3(kBlock), 0, s, d, r, L);
  }
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    if (weighted)
      go_w<MODE, VEC, CLAMPED, PT, LINEAR, true>(grid, s);
    else
      go_w<MODE, VEC, CLAMPED, PT, LINEAR, false>(grid, s);
  }
};
struct RdoqSkipLaunch { // rdoq_kernel's grid: the ladder's choice of VEC and of the linear or tiled grid is all it needs
  const EncDesc *d;
  const RdoqDesc *r;
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    hipLaunchKernelGGL((rdoq_skip_kernel<VEC, LINEAR>), grid, dim3(kBlock), 0, s, d, r);
  }
};
int launch_rdoq(const EncDesc *d_descs, const RdoqDesc *d_qdescs, const uint32_t *d_log2, bool weighted, bool skip, int count, int M_max, int64_t hw_max,
                int64_t n_max, bool linear, int mode, int vec, bool clamped, int planes, void *stream) {
  if (const int e = enc_launch<false>(RdoqLaunch{d_descs, d_qdescs, d_log2, weighted, skip}, count, M_max, hw_max, n_max, linear, mode, vec, clamped, planes, stream))
    return e;
  return skip ? enc_launch<false>(RdoqSkipLaunch{d_descs, d_qdescs}, count, M_max, hw_max, n_max, linear, mode, vec, clamped, planes, stream) : 0;
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
