// fgmm_rdoq.cpp — rate-distortion optimised quantisation of a batch of latents (include/flashgmm_amd.h sections 3c, 3e and 3f).  On the frame of
// fgmm_estimate.cpp (quant_stats_kernel and chan_compact_kernel give the channels the compress call would code for y): rdoq_kernel
// (fgmm_rdoq.hip) in place of rate_kernel, then the frame's second census, over y_rdo: its abs_max and zero_bitmap are what a compress
// call of y_rdo will return.  Nothing but the per-channel census and sums crosses PCIe.  A file of its own, as fgmm_estimate.cpp: the
// host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

// lambdas[i * lambda_stride] is item i's lambda (stride 0: one for the call, fgmm_gmc_rdoq_batch; 1: the budget call of section 3d, whose
// groups end at lambdas of their own): it travels in the item's RdoqDesc, so either way rdoq_kernel is launched once.
// sk non-null: section 3f - rdoq_kernel's SKIP form and rdoq_skip_kernel behind it, before the second census; the channels' words of both
// and the item's folded sums come back with the census, so the call gains no synchronisation
int fgmm::rdoq_run(fgmm_ctx *ctx, dev::Stream stream, fgmm_rdoq_item *items, int count, int mode, int clamp, const double *lambdas, int lambda_stride,
                   const fgmm_rdo_weights *w, bool w_check, fgmm_rdo_skip *sk) {
  LatentFrame fr(ctx, stream, latent_in(items, count), clamp);
  fr.w = w, fr.w_check = w_check;
  int rc;
  const size_t n_item = sk ? kRdoSkipItem : 0;
  // per channel: bits before | bits after | latents changed (| section 3f's words)
  if ((rc = fr.layout({sizeof(RdoqDesc), n_item, sk ? 3 + (size_t)kRdoSkipWords : 3, 0, true}))) return rc;
  RdoqDesc *hq = ws<RdoqDesc>(ctx->h_ws, fr.o_call);
  for (int i = 0; i < count; ++i) {
    hq[i].y_out = fr.out[(size_t)i] = items[i].y_rdo; // +0.0 where a channel is not coded (all of its round(y) are zeros)
    hq[i].item_sums = sk ? ws<unsigned long long>(ctx->d_ws, fr.o_back[(size_t)i]) : nullptr;
    hq[i].chan_before = ws<unsigned long long>(ctx->d_ws, fr.o_back[(size_t)i]) + n_item;
    hq[i].chan_after = hq[i].chan_before + items[i].M;
    hq[i].chan_changed = hq[i].chan_after + items[i].M;
    hq[i].chan_skip = sk ? hq[i].chan_changed + items[i].M : nullptr;
    hq[i].lam_q = lambdas[(size_t)i * lambda_stride] * 0x1p-24;
    hq[i].chan_w = fr.chan_w(i), hq[i].pos_w = fr.pos_w(i);
  }
  if ((rc = fr.start())) return rc;
  LAUNCH_TRY(launch_rdoq(fr.dd(), ws<const RdoqDesc>(ctx->d_ws, fr.o_call), ctx->d_rate_log2, fr.weighted, sk != nullptr, count, fr.M_max, fr.hw_max, fr.n_max, fr.linear,
                         mode, fr.vec, clamp != 0, fr.planes, stream));
  if ((rc = fr.finish(fr.o_small))) return rc; // (with the census of y_rdo)
  // ---- per item, on the host: the census of y_rdo as the compress call will read it (fgmm_encode.cpp side_info), the sums ------
  for (int i = 0; i < count; ++i) {
    fgmm_rdoq_item &it = items[i];
    const uint64_t *is = ws<const uint64_t>(ctx->h_ws, fr.o_back[(size_t)i]), *cb = is + n_item, *ca = cb + it.M, *cc = ca + it.M;
    (void)census_side_info(ctx, fr.census_out[(size_t)i], it.M, it.hw, it.zero_bitmap, &it.abs_max);
    uint64_t before = 0, after = 0, changed = 0;
    if (sk) { // the sums after the channel decisions: folded on the device, the channels' from the words rdoq_skip_kernel wrote
      const uint64_t *cs = cc + it.M;
      for (int c = 0; c < it.M; ++c) {
        if (it.chan_bits_q_after) it.chan_bits_q_after[c] = cs[(size_t)kRdoSkipAfter * it.M + c];
        if (sk[i].skipped) sk[i].skipped[c] = (int64_t)cs[(size_t)kRdoSkipFlag * it.M + c];
        before += cb[c];
      }
      it.n_changed = (int64_t)is[1];
      it.bits_q_before = before;
      it.bits_q_after = is[0];
      sk[i].ddist_q = is[2];
      sk[i].n_skipped = (int64_t)is[3];
      sk[i].n_eligible = (int64_t)is[4];
      it.status = FGMM_OK;
      continue;
    }
    for (int c = 0; c < it.M; ++c) {
      if (it.chan_bits_q_after) it.chan_bits_q_after[c] = ca[c];
      before += cb[c];
      after += ca[c];
      changed += cc[c];
    }
    it.n_changed = (int64_t)changed;
    it.bits_q_before = before;
    it.bits_q_after = after;
    it.status = FGMM_OK;
  }
  return FGMM_OK;
}

int fgmm::rdoq_check_items(const fgmm_rdoq_item *items, int count) {
  if (int rc = check_latent_items(latent_in(items, count))) return rc;
  for (int i = 0; i < count; ++i) {
    const fgmm_rdoq_item &s = items[i];
    if ((int64_t)s.M * s.hw && !s.y_rdo) return fail(FGMM_ERR_INVALID, "item %d: null tensor / negative size", i);
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(s.y), r0 = reinterpret_cast<uintptr_t>(s.y_rdo);
    const uintptr_t nb = sizeof(float) * (uintptr_t)s.M * (uintptr_t)s.hw; // (y_rdo is zeroed before the census reads y)
    if (nb && y0 < r0 + nb && r0 < y0 + nb) return fail(FGMM_ERR_INVALID, "item %d: y_rdo may not overlap y", i);
  }
  return FGMM_OK;
}

extern "C" {

int fgmm_gmc_rdoq_batch_s(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda,
                          const fgmm_rdo_weights *w, fgmm_rdo_skip *skip) {
  if (!(lambda >= 0.0 && lambda < (double)INFINITY)) return fail(FGMM_ERR_INVALID, "lambda = %g: must be finite and >= 0", lambda);
  if (!ctx || count < 0 || (count && !items) || mode < 0 || mode > 2) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = rdoq_check_items(items, count)) return rc;
  return latent_call(ctx, stream, items, count, [&](dev::Stream s) { return rdoq_run(ctx, s, items, count, mode, clamp_scales, &lambda, 0, w, true, skip); });
}
int fgmm_gmc_rdoq_batch_w(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda,
                          const fgmm_rdo_weights *w) {
  return fgmm_gmc_rdoq_batch_s(ctx, stream, items, count, mode, clamp_scales, lambda, w, nullptr);
}
int fgmm_gmc_rdoq_batch(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda) {
  return fgmm_gmc_rdoq_batch_w(ctx, stream, items, count, mode, clamp_scales, lambda, nullptr);
}

} // extern "C"
