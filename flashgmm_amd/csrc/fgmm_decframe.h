// fgmm_decframe.h — the one frame of the decode-side kernels of fgmm_tab.hip (tab_kernel, cdftab_count / cdftab_fill, segdec_kernel)
// and of their launchers: what they had each in a copy of their own.  Device code over any descriptor that names the planes as
// DecDesc and SegDesc do.
//   dec_channel               compact channel -> source channel
//   FGMM_DEC_PARAMS / _STORE  one latent's twelve parameters (softmax4 for logits), clamped sigma, reciprocals, the tame flag; ... as
//                             four float4 into the latent's LDS slot
//   tab_window, TrimState     the evaluation window between the saturated tails; the trimming of one row
//   FGMM_DEC_EVAL_PAIR        two consecutive quantised edges of a latent whose parameters lie in LDS: THE arithmetic of the tables
//   dec_launch                the launchers' ladder: plane type x clamped x mode -> DecRung<MODE, CLAMPED, PT>
// The three FGMM_DEC_* texts are MACROS: they expand where the kernels had them.  Every function form that was tried - by value, by
// reference, with functors for the kernels' own reads - changed the generated code of tab_kernel and segdec_kernel, some the
// registers of segdec_kernel (profiles/dec_frame_refactor.md has the list); a macro leaves all 74 kernels the text they had.
#pragma once
#include <algorithm>

#include "fgmm_dev.h"

namespace fgmm {

// GLOBAL: through ldg (the descriptor's pointers are generic: segdec_kernel keeps the lookup off the flat path)
template <bool GLOBAL = false, class D, class I> __device__ __forceinline__ int dec_channel(const D &d, I cj) {
  if constexpr (GLOBAL) return d.chan_list ? ldg<int32_t>(d.chan_list + cj) : (int)cj;
  else return d.chan_list ? d.chan_list[cj] : (int)cj;
}

// ---- one latent's parameters: latent p of channel c of descriptor d -> MU, SG, PI, RS (float[4] each) and TAME (bool) of the
// caller.  sg: sigma, clamped when CLAMPED; rs: its refined reciprocal (0 when not); tame: the packed evaluation is allowed - CLAMPED
// and no NaN sigma.  (TabLatent, the generic path, has its own scalar form of this: fgmm_tab.hip)
#define FGMM_DEC_PARAMS(CLAMPED, PT, d, c, p, MU, SG, PI, RS, TAME)                                                              \
  {                                                                                                                              \
    const int64_t base_ = (int64_t)(c) * (d).stride_c + (p) * (d).stride_p;                                                      \
    TAME = true;                                                                                                                 \
    _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                              \
      SG[k] = ld1<PT>((d).scales, base_ + k * (d).stride_k);                                                                     \
      MU[k] = ld1<PT>((d).means, base_ + k * (d).stride_k);                                                                      \
      PI[k] = ld1<PT>((d).weights, base_ + k * (d).stride_k);                                                                    \
    }                                                                                                                            \
    if ((d).logits) softmax4(PI);                                                                                                \
    if constexpr (CLAMPED) {                                                                                                     \
      Sigma4 S4_;                                                                                                                \
      S4_.set(SG[0], SG[1], SG[2], SG[3]);                                                                                       \
      TAME = S4_.tame;                                                                                                           \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                            \
        SG[k] = TAME ? S4_.sg[k] : clamp_scale(SG[k]); /* a NaN sigma stays NaN (the IEEE path is taken for this latent) */      \
        RS[k] = S4_.rs[k];                                                                                                       \
      }                                                                                                                          \
    } else {                                                                                                                     \
      TAME = false; /* un-clamped sigma: IEEE division, scalar evaluation */                                                     \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) RS[k] = 0.0f;                                                                \
    }                                                                                                                            \
  }
// slot l of P[.][4]: mu, sigma (clamped), pi, refined 1 / sigma
#define FGMM_DEC_PARAMS_STORE(P, l, MU, SG, PI, RS)                                                                              \
  {                                                                                                                              \
    (P)[4 * (l) + 0] = (float4_t){MU[0], MU[1], MU[2], MU[3]};                                                                   \
    (P)[4 * (l) + 1] = (float4_t){SG[0], SG[1], SG[2], SG[3]};                                                                   \
    (P)[4 * (l) + 2] = (float4_t){PI[0], PI[1], PI[2], PI[3]};                                                                   \
    (P)[4 * (l) + 3] = (float4_t){RS[0], RS[1], RS[2], RS[3]};                                                                   \
  }

// ---- evaluation window: skip the part of [-max_bs, max_bs+1] where every component is saturated -------------
// Saturation lemmas (fgmm_math.h Sat<MODE>, proved by exhaustive scan: fgmm_selftest_saturation):
//   all z_k <= -ZL  =>  F[v] == 0          all z_k >= +ZR  =>  F[v] == quant16((pi0+pi1)+(pi2+pi3))
// z_k(v) = ((float)v - 0.5f - mu_k) / sg_k is non-decreasing in v for finite mu and 0 < sg < inf (every IEEE
// operation is monotone), so it is enough to VERIFY the condition, with the kernel's own arithmetic, at one v:
// it then holds for every v beyond it.  Any latent whose parameters fall outside the lemmas' domain is
// evaluated over the full range instead.  Indices < j_lo are all zero, indices >= j_hi are all T_sat.
template <int MODE>
__device__ __forceinline__ void tab_window(const float (&mu)[4], const float (&sg)[4], const float (&pi)[4], int prune, int max_bs, int W,
                                           int &j_lo, int &j_hi, uint32_t &T_sat) {
  j_lo = 0;
  j_hi = W;
  T_sat = 0;
  if (prune) {
    bool ok = true;
    float tl = INFINITY, tr = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ok = ok && (sg[k] > 0.0f) && (sg[k] < INFINITY) && (fabsf(mu[k]) < INFINITY) && Sat<MODE>::weight_ok(pi[k]);
      tl = fminf(tl, __builtin_fmaf(-Sat<MODE>::ZL, sg[k], mu[k]));
      tr = fmaxf(tr, __builtin_fmaf(Sat<MODE>::ZR, sg[k], mu[k]));
    }
    if (ok) {
      const float lim = (float)max_bs + 4.0f;
      // left: largest candidate v with v - 0.5 <= tl, minus one for the rounding of tl itself
      const int vL = (int)fminf(fmaxf(floorf(tl + 0.5f) - 1.0f, -lim), lim);
      const int vR = (int)fminf(fmaxf(ceilf(tr + 0.5f) + 1.0f, -lim), lim);
      bool okL = true, okR = true;
      const float xl = (float)vL - 0.5f, xr = (float)vR - 0.5f;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        okL = okL && ((xl - mu[k]) / sg[k] <= -Sat<MODE>::ZL);
        okR = okR && ((xr - mu[k]) / sg[k] >= Sat<MODE>::ZR);
      }
      const int64_t lo = (int64_t)vL + max_bs + 1, hi = (int64_t)vR + max_bs;
      if (okL) j_lo = (int)std::min<int64_t>(std::max<int64_t>(lo, 0), W); // indices < j_lo are v <= vL: all zero
      if (okR) j_hi = (int)std::min<int64_t>(std::max<int64_t>(hi, j_lo), W); // indices >= j_hi are v >= vR: all T_sat
      T_sat = quant16((pi[0] + pi[1]) + (pi[2] + pi[3]));
    }
  }
}

// trimming state of one row, fed edge by edge in index order (both table paths run exactly this)
struct TrimState {
  int lead, run_start;
  bool allzero, nonmono;
  uint32_t prev;
  __device__ __forceinline__ void init(int j_lo) {
    lead = j_lo - 1;
    run_start = 0;
    allzero = true;
    nonmono = false;
    prev = 0;
  }
  __device__ __forceinline__ void step(int j, uint32_t E) {
    lead = (allzero && E == 0) ? j : lead; // index of the last leading zero
    allzero = allzero && E == 0;
    run_start = (j == 0 || E != prev) ? j : run_start;
    nonmono |= (j > 0) && (E < prev);
    prev = E;
  }
  // after the evaluated window: the saturated right part as one virtual step (F[j_hi .. W-1] == T_sat)
  __device__ __forceinline__ void finish(int j_hi, int W, uint32_t T_sat, int &a_idx, uint32_t &cnt) {
    if (j_hi < W) {
      if (allzero) {
        if (T_sat == 0) lead = W - 1; else allzero = false;
      }
      if (j_hi == 0 || T_sat != prev) run_start = j_hi;
      nonmono |= (j_hi > 0) && (T_sat < prev);
    }
    // the row starts at the first non-zero edge: F[v < a] = 0 is implied by the format, and the host takes "cf below the
    // first entry" as the interval [0, first entry) of the symbol before it
    a_idx = lead + 1;
    if (a_idx > run_start) a_idx = run_start;
    cnt = (uint32_t)(run_start - a_idx + 1);
  }
};

// ---- two consecutive edges F[j], F[j + 1] of the latent in slot l of P, quantised -> q0, q1 (uint32_t of the caller): what makes
// the decoder's tables the reference's, bit for bit, in tab_kernel and in segdec_kernel alike.  J and TAME are the kernel's own
// expressions over its window and flag words; they are evaluated where the kernels read those: J after the slot's four reads, TAME
// (CLAMPED only) in front of the packed evaluation.
#define FGMM_DEC_EVAL_PAIR(MODE, CLAMPED, P, l, J, TAME, max_bs, q0, q1)                                                         \
  {                                                                                                                              \
    const float4_t m4_ = (P)[4 * (l) + 0], s4_ = (P)[4 * (l) + 1], p4_ = (P)[4 * (l) + 2], r4_ = (P)[4 * (l) + 3];               \
    const float mu_[4] = {m4_[0], m4_[1], m4_[2], m4_[3]}, pi_[4] = {p4_[0], p4_[1], p4_[2], p4_[3]};                            \
    const int j_ = (J);                                                                                                          \
    const float x0_ = (float)(j_ - (max_bs)) - 0.5f, x1_ = (float)(j_ + 1 - (max_bs)) - 0.5f;                                    \
    float c0_ = 0.0f, c1_ = 0.0f;                                                                                                \
    bool fast_ = false;                                                                                                          \
    if constexpr (CLAMPED) {                                                                                                     \
      Sigma4 S4_;                                                                                                                \
      S4_.tame = true;                                                                                                           \
      _Pragma("unroll") for (int k = 0; k < 4; ++k) {                                                                            \
        S4_.sg[k] = s4_[k];                                                                                                      \
        S4_.rs[k] = r4_[k];                                                                                                      \
      }                                                                                                                          \
      bool ok_ = (TAME);                                                                                                         \
      const f2 cc_ = mix4_clamped2<MODE>((f2){x0_, x1_}, mu_, S4_, pi_, ok_);                                                    \
      c0_ = cc_.x;                                                                                                               \
      c1_ = cc_.y;                                                                                                               \
      fast_ = ok_;                                                                                                               \
    }                                                                                                                            \
    if (__builtin_expect(!fast_, 0)) { /* un-clamped sigma, NaN sigma, far-off or non-finite mean: IEEE evaluation */            \
      c0_ = mix4_slow<MODE>(x0_, mu_[0], mu_[1], mu_[2], mu_[3], s4_[0], s4_[1], s4_[2], s4_[3], pi_[0], pi_[1], pi_[2], pi_[3]); \
      c1_ = mix4_slow<MODE>(x1_, mu_[0], mu_[1], mu_[2], mu_[3], s4_[0], s4_[1], s4_[2], s4_[3], pi_[0], pi_[1], pi_[2], pi_[3]); \
    }                                                                                                                            \
    q0 = quant16(c0_);                                                                                                           \
    q1 = quant16(c1_);                                                                                                           \
  }

// ---- the launchers' ladder.  `mode` carries kPlanesBf16 (fgmm_internal.h: the plane type of a launch); f(DecRung<...>{}) launches
template <int M, bool C, typename T> struct DecRung {
  static constexpr int MODE = M;
  static constexpr bool CLAMPED = C;
  using PT = T;
};
template <bool CLAMPED, typename PT, typename F> static int dec_launch_m(const F &f, int mode) {
  switch (mode) {
  case MODE_AS: f(DecRung<MODE_AS, CLAMPED, PT>{}); break;
  case MODE_LOGISTIC: f(DecRung<MODE_LOGISTIC, CLAMPED, PT>{}); break;
  default: f(DecRung<MODE_POLYA, CLAMPED, PT>{}); break;
  }
  return (int)hipGetLastError();
}
template <typename F> static int dec_launch(const F &f, int mode, bool clamped, bool f16) {
  const bool bf16 = (mode & kPlanesBf16) != 0;
  mode &= kModeMask;
  if (bf16) return clamped ? dec_launch_m<true, __bf16>(f, mode) : dec_launch_m<false, __bf16>(f, mode);
  if (f16) return clamped ? dec_launch_m<true, _Float16>(f, mode) : dec_launch_m<false, _Float16>(f, mode);
  return clamped ? dec_launch_m<true, float>(f, mode) : dec_launch_m<false, float>(f, mode);
}

} // namespace fgmm
