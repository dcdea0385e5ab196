// fgmm_rdoq.hip — rate-distortion optimised quantisation of a latent (include/flashgmm_amd.h section 3c), for CDNA4 / gfx950 (MI355X).
//
//   rdoq_kernel   (y, sigma, mu, pi, lambda) -> per latent of a coded channel the symbol among round(y) - 1, round(y), round(y) + 1
//                 that minimises (y - v)^2 + lambda * bits(v), bits being the coder's own cost of v under that latent's mixture
//
// rdoq_kernel IS rate_kernel (fgmm_rate.hip) up to the loads - the same EncDesc addressing, both grids, the same softmax4 - and prices
// three symbols where rate_kernel prices one: the quantised CDF at the four edges v0 - 1.5 .. v0 + 1.5 (sym_edges4, fgmm_dev.h: two
// packed pairs sharing one Sigma4) gives the three table entries sym_entry would yield, each costs (16 << 24) - L[range] or the bypass
// escape's price of that symbol (rate_cost_q), and the objective is compared in binary64:
//   J(v) = d * d + lam_q * (double)cost_q(v),  d = (double)y - (double)v,  lam_q = lambda * 2^-24
// every operation a single IEEE operation (the file is built with -ffp-contract=off).  Start from v0; v0 - 1 if strictly smaller;
// then v0 + 1 if strictly smaller than the best so far: ties keep the earlier candidate, lambda = 0 returns round(y).  A latent
// that is not finite, or whose |v0| exceeds 2^20 (beyond it the edges of the neighbours are no longer the encoder's own), keeps v0.
// Sums (cost of v0, cost of the choice, latents moved) are integers: shuffles across the wave, one 64-bit atomic per wave and
// accumulator into the wave's channel, the same bits on every run.  52 B in (y + twelve planes), 4 B out per latent.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "fgmm_dev.h"

namespace fgmm {

constexpr float kRdoqMaxAbs = 0x1p20f;

// one latent of a coded channel -> the chosen symbol as a float (+0.0 for zero); cb / ca: cost of round(y) / of the choice
template <int MODE, bool CLAMPED>
__device__ __forceinline__ float rdoq_one(float y, const float (&mu)[4], const float (&sg)[4], const float (&pi)[4], double lam_q,
                                          const uint32_t *__restrict__ L, uint32_t &cb, uint32_t &ca) {
  const float vq = __builtin_rintf(y);
  const int vi = (int)vq;
  if (__builtin_expect(!(__builtin_fabsf(y) < INFINITY && __builtin_fabsf(vq) <= kRdoqMaxAbs), 0)) { // (false for NaN too)
    int bp;
    const uint32_t ent = sym_entry<MODE, CLAMPED>(vq, vi, mu, sg, pi, bp); // exactly rate_kernel's pricing
    cb = ca = entry_cost(ent, vq, vi, true, L);
    return vq + 0.0f;
  }
  uint32_t q[4];
  sym_edges4<MODE, CLAMPED>(vq, mu, sg, pi, q);
  int bp;
  const uint32_t cm = rate_cost_q(entry_from_edges(q[0], q[1], vi - 1, bp), vi - 1, L);
  const uint32_t c0 = rate_cost_q(entry_from_edges(q[1], q[2], vi, bp), vi, L);
  const uint32_t cp = rate_cost_q(entry_from_edges(q[2], q[3], vi + 1, bp), vi + 1, L);
  const float vm = vq - 1.0f, vp = vq + 1.0f;
  const double yd = (double)y;
  const double d0 = yd - (double)vq, dm = yd - (double)vm, dp = yd - (double)vp;
  const double j0 = d0 * d0 + lam_q * (double)c0;
  const double jm = dm * dm + lam_q * (double)cm;
  const double jp = dp * dp + lam_q * (double)cp;
  float v = vq;
  double jb = j0;
  cb = ca = c0;
  if (jm < jb) {
    v = vm;
    jb = jm;
    ca = cm;
  }
  if (jp < jb) {
    v = vp;
    ca = cp;
  }
  return v + 0.0f; // (-0.0 -> +0.0)
}

#ifndef FGMM_RDOQ_WAVES
#define FGMM_RDOQ_WAVES 4 // min waves per SIMD: 128 VGPRs - the four edges, three costs and the binary64 objective do not fit rate_kernel's 96
#endif
template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR>
__global__ __launch_bounds__(kBlock, FGMM_RDOQ_WAVES) void rdoq_kernel(const EncDesc *__restrict__ descs, const RdoqDesc *__restrict__ qdescs,
                                                                       const uint32_t *__restrict__ L, double lam_q) {
  const EncDesc &d = descs[blockIdx.z];
  const RdoqDesc &r = qdescs[blockIdx.z];
  const int64_t hw = d.hw;
  const int n_nz = d.chan_list[d.M]; // wave-uniform scalar load
  int rank;    // compact (coded) channel of this wave: wave-uniform in both grids
  int64_t p0;  // position of the lane's first latent within the channel
  bool active; // lanes past the end of a channel stay for the wave reduction
  if constexpr (LINEAR) { // every hw of the batch is a multiple of 64 * VEC: waves take 64 * VEC consecutive coded latents (rate_kernel)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w0 = ((int64_t)blockIdx.x * kBlock + wave * 64) * VEC;
    if (w0 >= (int64_t)n_nz * hw) return;
    rank = __builtin_amdgcn_readfirstlane((int)(w0 / hw));
    p0 = (w0 - (int64_t)rank * hw) + (int64_t)(threadIdx.x & 63) * VEC;
    active = true;
  } else { // one block per (tile of kBlock * VEC positions, compact channel)
    rank = blockIdx.y;
    if (rank >= n_nz) return;
    if ((int64_t)blockIdx.x * kBlock * VEC >= hw) return;
    p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    active = p0 < hw;
  }
  const int c = d.chan_list[rank];
  unsigned long long before = 0, after = 0; // the lane's latents (at most 4 * 52 bits each)
  int nchanged = 0;                         // the wave's, the same on every active lane (ballots)
  if (!active) {
  } else if constexpr (VEC > 1) {
    // planar, aligned (checked by the host): one VEC-wide load per plane per lane (16 B fp32 / 8 B fp16 at VEC = 4), one VEC-wide store
    typedef float fvec_t __attribute__((ext_vector_type(VEC)));
    const int64_t base = (int64_t)c * d.stride_c + p0;
    const fvec_t yv = ldg<fvec_t>(d.y + (int64_t)c * hw + p0);
    float S[4][VEC], Mu[4][VEC], Pi[4][VEC];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ldv<PT, VEC>(d.scales, base + k * d.stride_k, S[k]);
      ldv<PT, VEC>(d.means, base + k * d.stride_k, Mu[k]);
      ldv<PT, VEC>(d.weights, base + k * d.stride_k, Pi[k]);
    }
    fvec_t out;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        sg[k] = S[k][e];
        mu[k] = Mu[k][e];
        pi[k] = Pi[k][e];
      }
      if (d.logits) softmax4(pi);
      uint32_t cb, ca;
      out[e] = rdoq_one<MODE, CLAMPED>(yv[e], mu, sg, pi, lam_q, L, cb, ca);
      nchanged += __popcll(__ballot(out[e] != __builtin_rintf(yv[e]) && yv[e] == yv[e]));
      before += cb;
      after += ca;
    }
    stg<fvec_t>(r.y_out + (int64_t)c * hw + p0, out);
  } else {
    const int64_t base = (int64_t)c * d.stride_c + p0 * d.stride_p;
    const float y = ldg<float>(d.y + (int64_t)c * hw + p0);
    float mu[4], sg[4], pi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sg[k] = ld1<PT>(d.scales, base + k * d.stride_k);
      mu[k] = ld1<PT>(d.means, base + k * d.stride_k);
      pi[k] = ld1<PT>(d.weights, base + k * d.stride_k);
    }
    if (d.logits) softmax4(pi);
    uint32_t cb, ca;
    const float out = rdoq_one<MODE, CLAMPED>(y, mu, sg, pi, lam_q, L, cb, ca);
    nchanged = __popcll(__ballot(out != __builtin_rintf(y) && y == y));
    before = cb;
    after = ca;
    stg<float>(r.y_out + (int64_t)c * hw + p0, out);
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
template <int VEC, bool CLAMPED, typename PT, bool LINEAR>
static int launch_rdoq_v(const EncDesc *d, const RdoqDesc *r, const uint32_t *L, double lam_q, int count, int M_max, int64_t hw_max, int64_t n_max,
                         int mode, hipStream_t s) {
  const int64_t per_block = (int64_t)kBlock * VEC;
  const dim3 grid = LINEAR ? dim3((unsigned)((n_max + per_block - 1) / per_block), 1u, (unsigned)count)
                           : dim3((unsigned)((hw_max + per_block - 1) / per_block), (unsigned)M_max, (unsigned)count);
  switch (mode) {
  case MODE_AS: hipLaunchKernelGGL((rdoq_kernel<MODE_AS, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L, lam_q); break;
  case MODE_LOGISTIC: hipLaunchKernelGGL((rdoq_kernel<MODE_LOGISTIC, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L, lam_q); break;
  default: hipLaunchKernelGGL((rdoq_kernel<MODE_POLYA, VEC, CLAMPED, PT, LINEAR>), grid, dim3(kBlock), 0, s, d, r, L, lam_q); break;
  }
  return (int)hipGetLastError();
}
template <typename PT, bool LINEAR>
static int launch_rdoq_t(const EncDesc *d, const RdoqDesc *r, const uint32_t *L, double lam_q, int count, int M_max, int64_t hw_max, int64_t n_max,
                         int mode, int vec, bool clamped, hipStream_t s) {
  if (vec >= 4) return clamped ? launch_rdoq_v<4, true, PT, LINEAR>(d, r, L, lam_q, count, M_max, hw_max, n_max, mode, s)
                               : launch_rdoq_v<4, false, PT, LINEAR>(d, r, L, lam_q, count, M_max, hw_max, n_max, mode, s);
  return clamped ? launch_rdoq_v<1, true, PT, LINEAR>(d, r, L, lam_q, count, M_max, hw_max, n_max, mode, s)
                 : launch_rdoq_v<1, false, PT, LINEAR>(d, r, L, lam_q, count, M_max, hw_max, n_max, mode, s);
}

int launch_rdoq(const EncDesc *d_descs, const RdoqDesc *d_qdescs, const uint32_t *d_log2, double lam_q, int count, int M_max, int64_t hw_max,
                int64_t n_max, bool linear, int mode, int vec, bool clamped, bool f16, void *stream) {
  if (count <= 0 || M_max <= 0 || hw_max <= 0) return 0;
  if (count > 65535 || M_max > 65535) return (int)hipErrorInvalidValue; // grid.z, grid.y
  if (linear && (n_max + kBlock - 1) / kBlock > 0x7FFFFFFFll) linear = false; // grid.x
  hipStream_t s = (hipStream_t)stream;
  if (linear)
    return f16 ? launch_rdoq_t<_Float16, true>(d_descs, d_qdescs, d_log2, lam_q, count, M_max, hw_max, n_max, mode, vec, clamped, s)
               : launch_rdoq_t<float, true>(d_descs, d_qdescs, d_log2, lam_q, count, M_max, hw_max, n_max, mode, vec, clamped, s);
  return f16 ? launch_rdoq_t<_Float16, false>(d_descs, d_qdescs, d_log2, lam_q, count, M_max, hw_max, n_max, mode, vec, clamped, s)
             : launch_rdoq_t<float, false>(d_descs, d_qdescs, d_log2, lam_q, count, M_max, hw_max, n_max, mode, vec, clamped, s);
}

} // namespace fgmm
