// fgmm_encframe.h — the frame the three encode-side CDF kernels share: symtab_kernel (fgmm_kernels.hip), rate_kernel (fgmm_rate.hip)
// and rdoq_kernel (fgmm_rdoq.hip).  Where a wave sits in the linear and in the tiled grid, how the latent and the twelve parameter
// planes of an EncDesc are addressed and loaded for VEC = 1 / 2 / 4 / 8 positions per lane, how one position's (mu, sg, pi) is
// gathered before sym_entry, and the launchers' ladder over mode x VEC x clamped x plane type x grid.  A kernel adds only what it does
// with a position: the range one of them prices is the range the others code because they run this text, not a copy of it.
#pragma once
#include <type_traits>

#include "fgmm_dev.h"

namespace fgmm {

template <typename T, int N> struct vec_of { typedef T type __attribute__((ext_vector_type(N))); };

// ---------------------------------------------------------------------------------------------------------
// placement.  grid = (tiles over hw, compact channel j, item), or LINEAR: (tiles over the item's coded symbols, 1, item).  Rank j
// is the j-th NON-ZERO channel (chan_list, built on the device by chan_compact_kernel - entropy_models.py:844-845 channel
// compaction with no host round trip); a null chan_list is the raw (n, 4) building block: every channel, in order.
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int enc_n_coded(const EncDesc &d) { return d.chan_list ? d.chan_list[d.M] : d.M; } // wave-uniform scalar load
__device__ __forceinline__ int enc_channel(const EncDesc &d, int rank) { return d.chan_list ? d.chan_list[rank] : rank; }

// rank: compact (coded) channel of this wave - wave-uniform in both grids, so all addressing stays scalar; p0: position of the lane's
// first symbol within the channel; active: lanes past the end of a channel stay for the wave reductions (they are the wave's last
// ones: lane 0 is active whenever any lane is).  false: the wave has nothing to do and leaves.
template <int VEC, bool LINEAR>
__device__ __forceinline__ bool enc_place(int64_t hw, int n_nz, int &rank, int64_t &p0, bool &active) {
  if constexpr (LINEAR) {
    // Every hw of the batch is a multiple of 64 * VEC (checked by the host): the coded symbols of an item are one linear range
    // [0, n_nz * hw) and each WAVE takes 64 * VEC consecutive ones, never straddling a channel.  All waves are full whatever hw is
    // (a 768-symbol Kodak plane fills only 3 of the 4 waves of a per-channel block).
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t w0 = ((int64_t)blockIdx.x * kBlock + wave * 64) * VEC;
    if (w0 >= (int64_t)n_nz * hw) return false;
    rank = __builtin_amdgcn_readfirstlane((int)(w0 / hw));
    p0 = (w0 - (int64_t)rank * hw) + (int64_t)(threadIdx.x & 63) * VEC;
    active = true;
  } else {
    // one block per (tile of kBlock * VEC positions, compact channel); blocks with rank >= n_nz leave after one scalar load
    rank = blockIdx.y;
    if (rank >= n_nz) return false;
    if ((int64_t)blockIdx.x * kBlock * VEC >= hw) return false;
    p0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * VEC;
    active = p0 < hw;
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------
// loads and stores of VEC consecutive 4-byte values per lane: one VEC-wide access (16 B at VEC = 4), two 16-byte ones at VEC = 8
// ---------------------------------------------------------------------------------------------------------
template <typename T, int VEC> __device__ __forceinline__ void enc_ld(const T *p, T (&v)[VEC]) {
  constexpr int W = VEC > 4 ? 4 : VEC;
  typedef typename vec_of<T, W>::type vec_t;
#pragma unroll
  for (int h = 0; h < VEC; h += W) {
    const vec_t t = ldg<vec_t>(p + h);
#pragma unroll
    for (int e = 0; e < W; ++e) v[h + e] = t[e];
  }
}
template <typename T, int VEC> __device__ __forceinline__ void enc_st(T *p, const T (&v)[VEC]) {
  constexpr int W = VEC > 4 ? 4 : VEC;
  typedef typename vec_of<T, W>::type vec_t;
#pragma unroll
  for (int h = 0; h < VEC; h += W) {
    vec_t t;
#pragma unroll
    for (int e = 0; e < W; ++e) t[e] = v[h + e];
    stg<vec_t>(p + h, t);
  }
}

// the lane's latents: as they are (rdoq_kernel needs y itself) ...
template <int VEC> __device__ __forceinline__ void enc_load_y(const EncDesc &d, int c, int64_t p0, float (&y)[VEC]) {
  enc_ld<float, VEC>(d.y + (int64_t)c * d.hw + p0, y);
}
// ... or as the symbols to code, rounded latents or the raw boundary's symbols: vq = float(vi)
template <int VEC> __device__ __forceinline__ void enc_load_sym(const EncDesc &d, int c, int64_t p0, float (&vq)[VEC], int (&vi)[VEC]) {
  if (d.sym) {
    enc_ld<int, VEC>(d.sym + (int64_t)c * d.hw + p0, vi);
#pragma unroll
    for (int e = 0; e < VEC; ++e) vq[e] = (float)vi[e];
  } else {
    enc_load_y<VEC>(d, c, p0, vq);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      vq[e] = __builtin_rintf(vq[e]); // round-half-even == torch.round
      vi[e] = (int)vq[e];
    }
  }
}

// The twelve parameter planes of VEC positions of channel c: planar and aligned (checked by the host), one VEC-wide load per plane per
// lane - 16 B fp32 / 8 B fp16 or bf16 at VEC = 4, widened to float as they arrive.
// VEC = 8 (two-byte planes only, fp16 and bf16 alike): every plane read is ONE 16-byte load and the halves stay packed in registers (48 VGPRs for the twelve
// planes), widened as each position is evaluated.  Measured against VEC = 4 on ELIC-4K batches (profiles/r05_symtab_fp16_vec8_ab.txt):
// 127.6 / 133.1 against 123.0 / 126.8 G symbols per second (2 / 4 images) - symtab_kernel is bound by VALU issue (0.86 of the issue
// roof, bench.py's valu_frac) and this form issues fewer load and address instructions.
template <typename PT, int VEC> struct EncPlanes {
  typedef typename vec_of<PT, VEC>::type pvec_t;
  typedef typename vec_of<float, VEC>::type fvec_t;
  typedef typename std::conditional<VEC == 8, pvec_t, fvec_t>::type rvec_t;
  rvec_t S[4], Mu[4], Pi[4];
  static __device__ __forceinline__ rvec_t keep(pvec_t v) { // element by element, as ldv does
    rvec_t r;
#pragma unroll
    for (int e = 0; e < VEC; ++e) r[e] = v[e];
    return r;
  }
  __device__ __forceinline__ void load(const EncDesc &d, int c, int64_t p0) {
    const int64_t base = (int64_t)c * d.stride_c + p0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      S[k] = keep(ldg<pvec_t>(static_cast<const PT *>(d.scales) + base + k * d.stride_k));
      Mu[k] = keep(ldg<pvec_t>(static_cast<const PT *>(d.means) + base + k * d.stride_k));
      Pi[k] = keep(ldg<pvec_t>(static_cast<const PT *>(d.weights) + base + k * d.stride_k));
    }
  }
  // position e's mixture, the weights through softmax4 when the planes hold logits
  __device__ __forceinline__ void get(int e, int logits, float (&mu)[4], float (&sg)[4], float (&pi)[4]) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sg[k] = (float)S[k][e];
      mu[k] = (float)Mu[k][e];
      pi[k] = (float)Pi[k][e];
    }
    if (logits) softmax4(pi);
  }
};

// VEC = 1: scalars through stride_p (the raw (n, 4) rows).  Kept apart from the VEC-wide form, and the kernels leave their loop over
// the lane's positions by a `break` at VEC = 1 so that it is no loop to the compiler: with 1-wide vectors or a loop of one trip it lays
// `if (logits)` out as selects - softmax4 evaluated whether the planes hold logits or not - and takes up to 16 VGPRs more, an occupancy
// step for rdoq_kernel (profiles/enc_frame_refactor.md).
template <typename PT> struct EncPlanes<PT, 1> {
  float S[4], Mu[4], Pi[4];
  __device__ __forceinline__ void load(const EncDesc &d, int c, int64_t p0) {
    const int64_t base = (int64_t)c * d.stride_c + p0 * d.stride_p;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      S[k] = ld1<PT>(d.scales, base + k * d.stride_k);
      Mu[k] = ld1<PT>(d.means, base + k * d.stride_k);
      Pi[k] = ld1<PT>(d.weights, base + k * d.stride_k);
    }
  }
  __device__ __forceinline__ void get(int, int logits, float (&mu)[4], float (&sg)[4], float (&pi)[4]) const {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      sg[k] = S[k];
      mu[k] = Mu[k];
      pi[k] = Pi[k];
    }
    if (logits) softmax4(pi);
  }
};

// ---------------------------------------------------------------------------------------------------------
// The decision of include/flashgmm_amd.h sections 3c and 3e, shared by rdoq_kernel (fgmm_rdoq.hip: one lambda, the symbol written) and
// rdcurve_kernel (fgmm_rdcurve.hip: the same latent decided at up to 16 lambdas, nothing written): one text, so the two cannot drift.
// rdoq_price: a latent of a coded channel -> vq = round(y) and the exact costs cm, c0, cp of vq - 1, vq, vq + 1.  false: the latent is
// not finite or |vq| > 2^20 - it keeps round(y), and all three are rate_kernel's price of it.
// rdoq_choose: -1 / 0 / +1, the step 3c takes at lam_q = lambda * 2^-24.
// ---------------------------------------------------------------------------------------------------------
constexpr float kRdoqMaxAbs = 0x1p20f;
template <int MODE, bool CLAMPED>
__device__ __forceinline__ bool rdoq_price(float y, const float (&mu)[4], const float (&sg)[4], const float (&pi)[4], const uint32_t *__restrict__ L,
                                           float &vq, uint32_t &cm, uint32_t &c0, uint32_t &cp) {
  vq = __builtin_rintf(y);
  const int vi = (int)vq;
  if (__builtin_expect(!(__builtin_fabsf(y) < INFINITY && __builtin_fabsf(vq) <= kRdoqMaxAbs), 0)) { // (false for NaN too)
    int bp;
    const uint32_t ent = sym_entry<MODE, CLAMPED>(vq, vi, mu, sg, pi, bp); // exactly rate_kernel's pricing
    cm = c0 = cp = entry_cost(ent, vq, vi, true, L);
    return false;
  }
  uint32_t q[4];
  sym_edges4<MODE, CLAMPED>(vq, mu, sg, pi, q);
  int bp;
  cm = rate_cost_q(entry_from_edges(q[0], q[1], vi - 1, bp), vi - 1, L);
  c0 = rate_cost_q(entry_from_edges(q[1], q[2], vi, bp), vi, L);
  cp = rate_cost_q(entry_from_edges(q[2], q[3], vi + 1, bp), vi + 1, L);
  return true;
}
// d0, d: the distances (double)y - (double)v of round(y) and of the choice, for a caller that goes on with them.  wt: the latent's
// factor of section 3e, chan_w[c] * pos_w[p] as ONE binary64 product; 1.0 (a constant in the unweighted instantiations: the multiply
// folds away, and would change no bit if it stayed) gives 3c
__device__ __forceinline__ int rdoq_choose(float y, float vq, uint32_t cm, uint32_t c0, uint32_t cp, double lam_q, double wt, double &d0, double &d) {
  const float vm = vq - 1.0f, vp = vq + 1.0f;
  const double yd = (double)y;
  d0 = yd - (double)vq;
  const double dm = yd - (double)vm, dp = yd - (double)vp;
  const double j0 = wt * (d0 * d0) + lam_q * (double)c0;
  const double jm = wt * (dm * dm) + lam_q * (double)cm;
  const double jp = wt * (dp * dp) + lam_q * (double)cp;
  int pick = 0;
  double jb = j0;
  d = d0;
  if (jm < jb) {
    pick = -1;
    jb = jm;
    d = dm;
  }
  if (jp < jb) {
    pick = 1;
    d = dp;
  }
  return pick;
}
// The factors of section 3e as the weighted instantiations read them.  chan_w[c] is wave-uniform: a scalar load.  pos_w: the lane's VEC
// positions from p0, one VEC-wide load in POSITION index (no stride_p).  Every coded channel of an item reads the same hw floats again,
// so these are ordinary cached loads, not the frame's non-temporal ldg.  A null array: every factor 1
__device__ __forceinline__ float rdo_chan_w(const float *__restrict__ chan_w, int c) { return chan_w ? ((const FGMM_GLOBAL float *)chan_w)[c] : 1.0f; }
template <int VEC> __device__ __forceinline__ void rdo_pos_w(const float *__restrict__ pos_w, int64_t p0, float (&w)[VEC]) {
  static_assert(VEC == 1 || VEC == 4, "rdoq_kernel and rdcurve_kernel run 1 or 4 positions per lane");
  if (pos_w) { // (wave-uniform)
    if constexpr (VEC == 1) {
      w[0] = ((const FGMM_GLOBAL float *)pos_w)[p0];
    } else {
      const float4_t t = *(const FGMM_GLOBAL float4_t *)(pos_w + p0);
#pragma unroll
      for (int e = 0; e < VEC; ++e) w[e] = t[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < VEC; ++e) w[e] = 1.0f;
  }
}

// ---------------------------------------------------------------------------------------------------------
// Section 3f: the channel decision, ONE text for rdoq_skip_kernel and rdcurve_fold_kernel's skip form - every wave that asks about a
// channel runs the same binary64 sequence on the same integers.  rdo_skip_dz: a latent's term of Dz, in units of 2^-16
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool rdo_skip_rule(bool inelig, unsigned long long A, unsigned long long nzA, unsigned long long Dk, unsigned long long Dz,
                                              double lam_q) {
  if (inelig) return false;
  const double jk = (double)Dk * 0x1p-32 + lam_q * (double)A;
  const double jz = (double)Dz * 0x1p-16;
  return nzA == 0 || jz < jk;
}
__device__ __forceinline__ unsigned long long rdo_skip_dz(float y, float vq, double wt) { // (vq != 0, |vq| <= FGMM_SKIP_VMAX, y finite)
  const double dz = (double)y, d0 = (double)y - (double)vq;
  const double incz = dz * dz - d0 * d0;
  return (unsigned long long)(long long)__builtin_rint((wt * incz) * 0x1p16);
}

// ---------------------------------------------------------------------------------------------------------
// Section 3g's terms of one mixture component, ONE text for the likelihood kernels (fgmm_like.hip) and centroid_kernel
// (fgmm_centroid.hip, section 3i): s = max(sigma, sb) keeping a NaN sigma (LowerBound, bound_ops.py:36-37), the two standardised edges,
// p = u - l; and the density at an edge
// ---------------------------------------------------------------------------------------------------------
constexpr float kLikeC = (float)(-0.70710678118654752440);       // (float)(-(2^-0.5))            entropy_models.py:676
constexpr float kLikeInvSqrt2Pi = (float)0.39894228040143267794; // (float)(1 / sqrt(2 pi))
__device__ __forceinline__ float like_term(float v, float mu, float sigma, float sb, float &s, float &xu, float &xl) {
  s = max_nan(sigma, sb);
  const float a = __builtin_fabsf(v - mu);
  xu = (0.5f - a) / s;
  xl = (-0.5f - a) / s;
  const float u = 0.5f * erfcf(kLikeC * xu);
  const float l = 0.5f * erfcf(kLikeC * xl);
  return u - l;
}
__device__ __forceinline__ float like_phi(float x) { return expf(-0.5f * x * x) * kLikeInvSqrt2Pi; }

// ---------------------------------------------------------------------------------------------------------
// the ladder of the kernels without a mode (like_kernel, like_bwd_kernel, centroid_kernel): VEC (1, 4, and 8 for two-byte planes where
// F::kVec8 says the kernel has it) x plane type x grid.  F::go<VEC, PT, LINEAR>(grid, stream) does the kernel's hipLaunchKernelGGL
// ---------------------------------------------------------------------------------------------------------
template <int VEC, typename PT, bool LINEAR, typename F> static int like_launch_v(const F &f, int count, int M_max, int64_t hw_max, int64_t n_max, hipStream_t s) {
  const int64_t per_block = (int64_t)kBlock * VEC;
  const dim3 grid = LINEAR ? dim3((unsigned)((n_max + per_block - 1) / per_block), 1u, (unsigned)count)
                           : dim3((unsigned)((hw_max + per_block - 1) / per_block), (unsigned)M_max, (unsigned)count);
  f.template go<VEC, PT, LINEAR>(grid, s);
  return (int)hipGetLastError();
}
template <typename PT, bool LINEAR, typename F> static int like_launch_t(const F &f, int count, int M_max, int64_t hw_max, int64_t n_max, int vec, hipStream_t s) {
  if constexpr (F::kVec8 && sizeof(PT) == 2)
    if (vec == 8) return like_launch_v<8, PT, LINEAR>(f, count, M_max, hw_max, n_max, s);
  if (vec >= 4) return like_launch_v<4, PT, LINEAR>(f, count, M_max, hw_max, n_max, s);
  return like_launch_v<1, PT, LINEAR>(f, count, M_max, hw_max, n_max, s);
}
template <typename F> static int like_launch(const F &f, int count, int M_max, int64_t hw_max, int64_t n_max, bool linear, int vec, int planes, void *stream) {
  if (count <= 0 || M_max <= 0 || hw_max <= 0) return 0;
  if (linear && (n_max + kBlock - 1) / kBlock > 0x7FFFFFFFll) linear = false;        // grid.x
  if (count > 65535 || (!linear && M_max > 65535)) return (int)hipErrorInvalidValue; // grid.z; grid.y is M_max on the tiled grid only
  hipStream_t s = (hipStream_t)stream;
  if (planes == FGMM_BF16)
    return linear ? like_launch_t<__bf16, true>(f, count, M_max, hw_max, n_max, vec, s) : like_launch_t<__bf16, false>(f, count, M_max, hw_max, n_max, vec, s);
  if (planes == FGMM_F16)
    return linear ? like_launch_t<_Float16, true>(f, count, M_max, hw_max, n_max, vec, s) : like_launch_t<_Float16, false>(f, count, M_max, hw_max, n_max, vec, s);
  return linear ? like_launch_t<float, true>(f, count, M_max, hw_max, n_max, vec, s) : like_launch_t<float, false>(f, count, M_max, hw_max, n_max, vec, s);
}

// ---------------------------------------------------------------------------------------------------------
// the launchers' ladder.  F::go<MODE, VEC, CLAMPED, PT, LINEAR>(grid, stream) does the kernel's hipLaunchKernelGGL with its own
// arguments.  ALL_VEC: VEC = 2, and 8 for two-byte planes, exist too (symtab_kernel's A/B forms and its fp16 / bf16 default); else vec >= 4 is 4
// and anything below is 1.  M_max, hw_max, n_max: the largest M, hw and M * hw of the batch.
// ---------------------------------------------------------------------------------------------------------
template <int VEC, bool CLAMPED, typename PT, bool LINEAR, typename F> static int enc_launch_m(const F &f, dim3 grid, int mode, hipStream_t s) {
  switch (mode) {
  case MODE_AS: f.template go<MODE_AS, VEC, CLAMPED, PT, LINEAR>(grid, s); break;
  case MODE_LOGISTIC: f.template go<MODE_LOGISTIC, VEC, CLAMPED, PT, LINEAR>(grid, s); break;
  default: f.template go<MODE_POLYA, VEC, CLAMPED, PT, LINEAR>(grid, s); break;
  }
  return (int)hipGetLastError();
}
template <int VEC, typename PT, bool LINEAR, typename F>
static int enc_launch_v(const F &f, int count, int M_max, int64_t hw_max, int64_t n_max, int mode, bool clamped, hipStream_t s) {
  const int64_t per_block = (int64_t)kBlock * VEC;
  const dim3 grid = LINEAR ? dim3((unsigned)((n_max + per_block - 1) / per_block), 1u, (unsigned)count)
                           : dim3((unsigned)((hw_max + per_block - 1) / per_block), (unsigned)M_max, (unsigned)count);
  return clamped ? enc_launch_m<VEC, true, PT, LINEAR>(f, grid, mode, s) : enc_launch_m<VEC, false, PT, LINEAR>(f, grid, mode, s);
}
template <bool ALL_VEC, typename PT, bool LINEAR, typename F>
static int enc_launch_t(const F &f, int count, int M_max, int64_t hw_max, int64_t n_max, int mode, int vec, bool clamped, hipStream_t s) {
  if constexpr (ALL_VEC && sizeof(PT) == 2) // (two-byte planes only: 16-byte loads per plane)
    if (vec == 8) return enc_launch_v<8, PT, LINEAR>(f, count, M_max, hw_max, n_max, mode, clamped, s);
  if (vec >= 4) return enc_launch_v<4, PT, LINEAR>(f, count, M_max, hw_max, n_max, mode, clamped, s);
  if constexpr (ALL_VEC)
    if (vec == 2) return enc_launch_v<2, PT, LINEAR>(f, count, M_max, hw_max, n_max, mode, clamped, s);
  return enc_launch_v<1, PT, LINEAR>(f, count, M_max, hw_max, n_max, mode, clamped, s);
}
// planes: the fgmm_dtype of the parameter planes
template <bool ALL_VEC, typename F>
static int enc_launch(const F &f, int count, int M_max, int64_t hw_max, int64_t n_max, bool linear, int mode, int vec, bool clamped, int planes,
                      void *stream) {
  if (count <= 0 || M_max <= 0 || hw_max <= 0) return 0;
  if (linear && (n_max + kBlock - 1) / kBlock > 0x7FFFFFFFll) linear = false; // grid.x
  if (count > 65535 || (!linear && M_max > 65535)) return (int)hipErrorInvalidValue; // grid.z; grid.y is M_max on the tiled grid only
  hipStream_t s = (hipStream_t)stream;
  if (planes == FGMM_BF16)
    return linear ? enc_launch_t<ALL_VEC, __bf16, true>(f, count, M_max, hw_max, n_max, mode, vec, clamped, s)
                  : enc_launch_t<ALL_VEC, __bf16, false>(f, count, M_max, hw_max, n_max, mode, vec, clamped, s);
  const bool f16 = planes == FGMM_F16;
  if (linear)
    return f16 ? enc_launch_t<ALL_VEC, _Float16, true>(f, count, M_max, hw_max, n_max, mode, vec, clamped, s)
               : enc_launch_t<ALL_VEC, float, true>(f, count, M_max, hw_max, n_max, mode, vec, clamped, s);
  return f16 ? enc_launch_t<ALL_VEC, _Float16, false>(f, count, M_max, hw_max, n_max, mode, vec, clamped, s)
             : enc_launch_t<ALL_VEC, float, false>(f, count, M_max, hw_max, n_max, mode, vec, clamped, s);
}

} // namespace fgmm
