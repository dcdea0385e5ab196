// fgmm_rdcurve.hip — a stretch of the rate-distortion curve of a latent in one pass (include/flashgmm_amd.h section 3d), for CDNA4 / gfx950
// (MI355X).
//
//   rdcurve_kernel  (y, sigma, mu, pi, up to 16 lambdas) -> per channel and lambda what rdoq_kernel would sum at that lambda: the cost of
//                   the chosen symbols, the latents moved, the distortion the moves add.  Nothing is written per latent
//   rdcurve_fold_kernel  the channels' sums -> the item's; its skip form makes section 3f's decision per (channel, lambda) first
//
// The fourth kernel on the encode frame (fgmm_encframe.h).  Placement, loads and pricing are rdoq_kernel's (enc_place, enc_load_y,
// EncPlanes, rdoq_price): 52 B in per latent, 0 out.  Once a latent is priced the lane keeps of it y, round(y) and three costs - five
// registers - and the twelve plane registers are dead; the decision at one more lambda (rdoq_choose, the text rdoq_kernel runs) is a
// few binary64 operations on those five and no memory traffic.  The lambdas are the item's (RdCurveDesc, read by scalar loads once per
// wave and lambda: a budget search gives every group of items its own grid in one launch).
//   Registers: sixteen sets of per-lane 64-bit sums do not fit beside the pricing (rdoq_kernel holds 106-112 VGPRs at VEC = 4 under
// the same 4-waves-per-SIMD bound).  Each lambda is therefore reduced across the wave as it is evaluated (wave_sum64, the moves by
// ballots) and the wave's three results are kept by ONE lane, lane j for lambda j: three accumulators per lane in all.  After the
// loop lanes 0 .. n - 1 add their results into the channel's row with one 64-bit atomic each (integers: the same bits on every run).
#include <hip/hip_runtime.h>

#include "fgmm_encframe.h"

namespace fgmm {

#ifndef FGMM_RDCURVE_WAVES
#define FGMM_RDCURVE_WAVES 4 // min waves per SIMD, as rdoq_kernel: the pricing is the same
#endif
// WEIGHTED: section 3e, as rdoq_kernel's.  The lane keeps the FLOAT factor of each of its positions (VEC registers, not 2 * VEC) and the
// channel's in a scalar; their binary64 product is formed inside the lambda loop - exact, so where it is formed changes no bit.
// SKIP: section 3f.  Dz, nz0 and inelig need only y, round(y) and the factor: taken once per wave BEFORE the lambda loop and reduced at
// once, so that they hold no register inside it.  nzA is per lambda, a ballot count as the moves are; the two counts (each at most
// 64 * VEC per wave) share lane j's third accumulator, moves in the low half, so the loop carries no fourth (profiles/rdo_skip.md)
template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR, bool WEIGHTED, bool SKIP>
__global__ __launch_bounds__(kBlock, FGMM_RDCURVE_WAVES) void rdcurve_kernel(const EncDesc *__restrict__ descs, const RdCurveDesc *__restrict__ cdescs,
                                                                             const uint32_t *__restrict__ L) {
  const RdCurveDesc &r = cdescs[blockIdx.z];
  const int n = r.n_lambda; // (0: the item takes no part in this pass)
  if (n <= 0) return;
  const EncDesc &d = descs[blockIdx.z];
  const int64_t hw = d.hw;
  int rank;
  int64_t p0;
  bool active;
  if (!enc_place<VEC, LINEAR>(hw, d.chan_list[d.M], rank, p0, active)) return;
  const int c = d.chan_list[rank];
  // the lane's priced latents.  A lane past the end of its channel holds latents that cost nothing and never move
  float y[VEC], vq[VEC];
  uint32_t cm[VEC], c0[VEC], cp[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) y[e] = vq[e] = 0.0f, cm[e] = c0[e] = cp[e] = 0u;
  unsigned long long before = 0;
  float cw = 1.0f, pw[VEC];
#pragma unroll
  for (int e = 0; e < VEC; ++e) pw[e] = 1.0f;
  bool bad = false; // SKIP: a latent of the lane that is not priced (not finite, or beyond 2^20)
  if (active) {
    if constexpr (WEIGHTED) {
      cw = rdo_chan_w(r.chan_w, c);
      rdo_pos_w<VEC>(r.pos_w, p0, pw);
    }
    enc_load_y<VEC>(d, c, p0, y);
    EncPlanes<PT, VEC> P;
    P.load(d, c, p0);
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      float mu[4], sg[4], pi[4];
      P.get(e, d.logits, mu, sg, pi);
      const bool priced = rdoq_price<MODE, CLAMPED>(y[e], mu, sg, pi, L, vq[e], cm[e], c0[e], cp[e]);
      if (!priced) y[e] = vq[e] = 0.0f; // keeps round(y) at every lambda: three equal costs at distance 0, 1, 1
      if constexpr (SKIP) bad = bad || !priced;
      before += c0[e];
      if constexpr (VEC == 1) break; // (one position: no loop, see EncPlanes<PT, 1>)
    }
  }
  before = wave_sum64(before);
  if (!before) return; // (every symbol costs something: 0 = a wave wholly past the end of its channel; wave-uniform)
  const int lane = threadIdx.x & 63;
  constexpr int kRow = SKIP ? kRdCurveRowS : kRdCurveRow;
  unsigned long long *row = r.chan_acc + (int64_t)c * kRow;
  if constexpr (SKIP) { // (a latent that is not priced makes its channel ineligible: what its zeroed y and vq leave out is never looked at)
    unsigned long long dz = 0;
    int nz0 = 0;
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      const bool nz = vq[e] != 0.0f, big = __builtin_fabsf(vq[e]) > (float)FGMM_SKIP_VMAX;
      nz0 += __popcll(__ballot(nz));
      bad = bad || big;
      if (nz && !big) {
        double wt = 1.0;
        if constexpr (WEIGHTED) wt = (double)cw * (double)pw[e];
        dz += rdo_skip_dz(y[e], vq[e], wt);
      }
      if constexpr (VEC == 1) break;
    }
    dz = wave_sum64(dz);
    const bool inel = __ballot(bad) != 0;
    if (lane == 0) {
      if (dz) add64(row + kRdCurveRow + FGMM_RDCURVE_MAX, dz);
      if (nz0) add64(row + kRdCurveRow + FGMM_RDCURVE_MAX + 1, (unsigned long long)nz0);
      if (inel) add64(row + kRdCurveRow + FGMM_RDCURVE_MAX + 2, 1ull);
    }
  }
  unsigned long long r_after = 0, r_dd = 0, r_changed = 0; // lane j: the wave's sums at lambda j
  for (int j = 0; j < n; ++j) {
    const double lam_q = r.lam_q[j]; // wave-uniform: a scalar load
    unsigned long long after = 0, dd = 0;
    int changed = 0; // the wave's, the same on every lane (ballots)
    int nza = 0;     // SKIP: the wave's latents whose choice is not 0
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      double d0, dv, wt = 1.0;
      if constexpr (WEIGHTED) wt = (double)cw * (double)pw[e];
      const int pick = rdoq_choose(y[e], vq[e], cm[e], c0[e], cp[e], lam_q, wt, d0, dv);
      after += pick < 0 ? cm[e] : pick > 0 ? cp[e] : c0[e];
      changed += __popcll(__ballot(pick != 0));
      if constexpr (SKIP) nza += __popcll(__ballot(vq[e] + (float)pick != 0.0f));
      if (pick) { // what the move adds to the (weighted) squared error, in units of 2^-32, rounded half to even: an integer, so the sum has no order
        const double inc = dv * dv - d0 * d0;
        dd += (unsigned long long)(long long)__builtin_rint((wt * inc) * 0x1p32);
      }
      if constexpr (VEC == 1) break;
    }
    after = wave_sum64(after);
    if (changed) dd = wave_sum64(dd); // (wave-uniform)
    if (lane == j) r_after = after, r_dd = dd, r_changed = (unsigned long long)changed | (unsigned long long)nza << 32; // (nza: 0 without SKIP)
  }
  if (lane == 0) add64(row, before);
  if (lane < n) {
    add64(row + 1 + lane, r_after);
    if constexpr (SKIP) {
      if (r_changed >> 32) add64(row + kRdCurveRow + lane, r_changed >> 32);
      r_changed &= 0xFFFFFFFFull;
    }
    if (r_changed) {
      add64(row + 1 + FGMM_RDCURVE_MAX + lane, r_changed);
      add64(row + 1 + 2 * FGMM_RDCURVE_MAX + lane, r_dd);
    }
  }
}

// the item's sums from its channels': block = (item), thread t of slice s adds the channels s, s + 4 ... of column t
__global__ __launch_bounds__(kBlock) void rdcurve_fold_kernel(const EncDesc *__restrict__ descs, const RdCurveDesc *__restrict__ cdescs) {
  const RdCurveDesc &r = cdescs[blockIdx.x];
  if (r.n_lambda <= 0) return;
  const int M = descs[blockIdx.x].M;
  const int t = threadIdx.x & 63, s = threadIdx.x >> 6;
  if (t >= kRdCurveRow) return;
  unsigned long long v = 0;
  for (int c = s; c < M; c += kBlock / 64) v += r.chan_acc[(int64_t)c * kRdCurveRow + t];
  if (v) add64(r.sums + t, v);
}

// section 3f's form: the decision per (channel, lambda) on the device, by rdo_skip_rule, then the item's sums after it.  Thread j < n
// of slice s decides the channels s, s + 4 ... at lambda j; thread 16 adds bits_q_before and counts the eligible channels
__global__ __launch_bounds__(kBlock) void rdcurve_fold_skip_kernel(const EncDesc *__restrict__ descs, const RdCurveDesc *__restrict__ cdescs) {
  const RdCurveDesc &r = cdescs[blockIdx.x];
  const int n = r.n_lambda;
  if (n <= 0) return;
  const int M = descs[blockIdx.x].M;
  const bool hw_big = descs[blockIdx.x].hw > (1ll << 24);
  const int t = threadIdx.x & 63, s = threadIdx.x >> 6;
  if (t > FGMM_RDCURVE_MAX || (t < FGMM_RDCURVE_MAX && t >= n)) return;
  unsigned long long after = 0, changed = 0, dd = 0, skipped = 0; // thread 16: `after` is bits_q_before, `skipped` the eligible channels
  for (int c = s; c < M; c += kBlock / 64) {
    const unsigned long long *row = r.chan_acc + (int64_t)c * kRdCurveRowS, *x = row + kRdCurveRow + FGMM_RDCURVE_MAX;
    if (!row[0]) continue; // not coded
    const bool inelig = x[2] != 0 || hw_big;
    if (t == FGMM_RDCURVE_MAX) {
      after += row[0];
      skipped += inelig ? 0 : 1;
      continue;
    }
    const unsigned long long A = row[1 + t], Dk = row[1 + 2 * FGMM_RDCURVE_MAX + t];
    if (rdo_skip_rule(inelig, A, row[kRdCurveRow + t], Dk, x[0], r.lam_q[t])) {
      changed += x[1];
      dd += x[0] << 16;
      skipped += 1;
    } else {
      after += A;
      changed += row[1 + FGMM_RDCURVE_MAX + t];
      dd += Dk;
    }
  }
  if (t == FGMM_RDCURVE_MAX) {
    if (after) add64(r.sums, after);
    if (skipped) add64(r.sums + kRdCurveRow + FGMM_RDCURVE_MAX, skipped);
    return;
  }
  if (after) add64(r.sums + 1 + t, after);
  if (changed) add64(r.sums + 1 + FGMM_RDCURVE_MAX + t, changed);
  if (dd) add64(r.sums + 1 + 2 * FGMM_RDCURVE_MAX + t, dd);
  if (skipped) add64(r.sums + kRdCurveRow + t, skipped);
}

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
struct RdCurveLaunch {
  const EncDesc *d;
  const RdCurveDesc *r;
  const uint32_t *L;
  bool weighted, skip;
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR, bool WEIGHTED> void go_w(dim3 grid, hipStream_t s) const {
    if (skip)
      hipLaunchKernelGGL((rdcurve_kernel<MODE, VEC, CLAMPED, PT, LINEAR, WEIGHTED, true>), grid, dim3(kBlock), 0, s, d, r, L);
    else
      hipLaunchKernelGGL((rdcurve_kernel<MODE, VEC, CLAMPED, PT, LINEAR, WEIGHTED, false>), grid, dim3(kBlock), 0, s, d, r, L);
  }
  template <int MODE, int VEC, bool CLAMPED, typename PT, bool LINEAR> void go(dim3 grid, hipStream_t s) const {
    if (weighted)
      go_w<MODE, VEC, CLAMPED, PT, LINEAR, true>(grid, s);
    else
      go_w<MODE, VEC, CLAMPED, PT, LINEAR, false>(grid, s);
  }
};
int launch_rdcurve(const EncDesc *d_descs, const RdCurveDesc *d_cdescs, const uint32_t *d_log2, bool weighted, bool skip, int count, int M_max, int64_t hw_max, int64_t n_max,
                   bool linear, int mode, int vec, bool clamped, int planes, void *stream) {
  if (count <= 0 || M_max <= 0 || hw_max <= 0) return 0;
  if (const int e = enc_launch<false>(RdCurveLaunch{d_descs, d_cdescs, d_log2, weighted, skip}, count, M_max, hw_max, n_max, linear, mode, vec, clamped, planes, stream)) return e;
  if (skip)
    hipLaunchKernelGGL(rdcurve_fold_skip_kernel, dim3((unsigned)count), dim3(kBlock), 0, (hipStream_t)stream, d_descs, d_cdescs);
  else
    hipLaunchKernelGGL(rdcurve_fold_kernel, dim3((unsigned)count), dim3(kBlock), 0, (hipStream_t)stream, d_descs, d_cdescs);
  return (int)hipGetLastError();
}

} // namespace fgmm
