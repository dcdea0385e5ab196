// fgmm_like.cpp — the entropy model's forward(): the likelihood of a batch of latents, its rate, and the gradients of either
// (include/flashgmm_amd.h section 3g, and 3h: the same on the parameter head's logits, the softmax over K and its derivative in the
// kernels).  Orchestration over fgmm_like.hip behind two entry points per section, in the shell of the pricing calls
// (fgmm_ctx.h: latent_call, check_latent_items) but without their census front half: every channel is evaluated.  Per call, whatever
// the number of items: one upload of descriptors, one memset of the sums, one launch, one small copy back.  A file of its own: the
// host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

namespace {

// (like_desc and LikeShape, an item's EncDesc and the batch's load width and grid, are fgmm_ctx.h's: the centroid call decides the same way)

// logits: the call is section 3h's.  One call is one form: every item carries exactly the flags of its section
template <class Item> int like_check(const Item *items, int count, float scale_bound, float likelihood_bound, bool logits) {
  if (!(scale_bound > 0.0f) || !(scale_bound < INFINITY)) return fail(FGMM_ERR_INVALID, "scale_bound = %g: must be positive and finite", (double)scale_bound);
  if (!(likelihood_bound >= 0.0f) || !(likelihood_bound < INFINITY))
    return fail(FGMM_ERR_INVALID, "likelihood_bound = %g: must be finite and >= 0", (double)likelihood_bound);
  if (int rc = check_latent_items(latent_in(items, count))) return rc;
  for (int i = 0; i < count; ++i) {
    if (logits && items[i].params.flags != FGMM_PARAMS_LOGITS)
      return fail(FGMM_ERR_INVALID, "item %d: fgmm_params.flags must be FGMM_PARAMS_LOGITS (the weights planes of this call hold logits)", i);
    if (!logits && items[i].params.flags) // section 3g: the softmax over K stays the caller's, so that autograd differentiates it
      return fail(FGMM_ERR_INVALID, "item %d: fgmm_params.flags must be 0 (FGMM_PARAMS_LOGITS is not taken here)", i);
    if (!items[i].y) return fail(FGMM_ERR_INVALID, "item %d: null y", i);
  }
  return FGMM_OK;
}

int likelihood_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_like_item *items, int count, int round, float sb, float lb, bool logits) {
  Arena ar;
  const size_t o_descs = ar.take(sizeof(EncDesc) * (size_t)count), o_call = ar.take(sizeof(LikeDesc) * (size_t)count);
  const size_t o_sums = ar.take(2 * sizeof(uint64_t) * (size_t)count), end = ar.off;
  int rc;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(end)) || (rc = ctx->ensure_events(1))) return rc;
  EncDesc *hd = ws<EncDesc>(ctx->h_ws, o_descs);
  LikeDesc *hl = ws<LikeDesc>(ctx->h_ws, o_call);
  LikeShape sh;
  const int planes = items[0].params.dtype;
  for (int i = 0; i < count; ++i) {
    const fgmm_like_item &it = items[i];
    like_desc(hd[i], it.y, it.params, it.M, it.hw);
    hl[i] = LikeDesc{it.like_out, it.v_out, ws<unsigned long long>(ctx->d_ws, o_sums) + 2 * i};
    sh.item(hd[i], planes_two_byte(planes), {it.like_out, it.v_out});
  }
  sh.done(hd, count, 8);
  DEV_TRY(dev::copy_async(ctx->d_ws + o_descs, hd, o_sums - o_descs, dev::kH2D, stream)); // (both descriptor arrays: one copy)
  DEV_TRY(dev::memset_async(ctx->d_ws + o_sums, 0, end - o_sums, stream));
  LAUNCH_TRY(launch_like(ws<const EncDesc>(ctx->d_ws, o_descs), ws<const LikeDesc>(ctx->d_ws, o_call), round, sb, lb, count, sh.M_max, sh.hw_max, sh.n_max,
                         sh.linear, sh.vec, planes, logits, stream));
  DEV_TRY(dev::copy_async(ctx->h_ws + o_sums, ctx->d_ws + o_sums, end - o_sums, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  const uint64_t *sums = ws<const uint64_t>(ctx->h_ws, o_sums);
  for (int i = 0; i < count; ++i) {
    items[i].bits_q = (int64_t)sums[2 * i];
    items[i].n_nonfinite = (int64_t)sums[2 * i + 1];
    items[i].status = FGMM_OK;
  }
  return FGMM_OK;
}

int likelihood_backward_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_like_grad_item *items, int count, int round, float sb, float lb,
                              bool logits) {
  Arena ar;
  const size_t o_descs = ar.take(sizeof(EncDesc) * (size_t)count), o_call = ar.take(sizeof(LikeGradDesc) * (size_t)count), end = ar.off;
  int rc;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(end)) || (rc = ctx->ensure_events(1))) return rc;
  EncDesc *hd = ws<EncDesc>(ctx->h_ws, o_descs);
  LikeGradDesc *hg = ws<LikeGradDesc>(ctx->h_ws, o_call);
  LikeShape sh;
  const int planes = items[0].params.dtype;
  for (int i = 0; i < count; ++i) {
    const fgmm_like_grad_item &it = items[i];
    like_desc(hd[i], it.y, it.params, it.M, it.hw);
    hg[i] = LikeGradDesc{it.g_like, (float)it.g_bits, it.dy, it.dscales, it.dmeans, it.dweights};
    sh.item(hd[i], planes_two_byte(planes), {it.g_like, it.dy, it.dscales, it.dmeans, it.dweights});
  }
  sh.done(hd, count, 4);
  DEV_TRY(dev::copy_async(ctx->d_ws + o_descs, hd, end - o_descs, dev::kH2D, stream));
  LAUNCH_TRY(launch_like_bwd(ws<const EncDesc>(ctx->d_ws, o_descs), ws<const LikeGradDesc>(ctx->d_ws, o_call), round, sb, lb, count, sh.M_max, sh.hw_max,
                             sh.n_max, sh.linear, sh.vec, planes, logits, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  for (int i = 0; i < count; ++i) items[i].status = FGMM_OK;
  return FGMM_OK;
}

// the two entry points of a section: its validation, then the shell
int likelihood_entry(fgmm_ctx *ctx, void *stream, fgmm_like_item *items, int count, int round, float scale_bound, float likelihood_bound, bool logits) {
  if (!ctx || count < 0 || (count && !items)) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = like_check(items, count, scale_bound, likelihood_bound, logits)) return rc;
  return latent_call(ctx, stream, items, count,
                     [&](dev::Stream s) { return likelihood_batch(ctx, s, items, count, round != 0, scale_bound, likelihood_bound, logits); });
}

int likelihood_backward_entry(fgmm_ctx *ctx, void *stream, fgmm_like_grad_item *items, int count, int round, float scale_bound, float likelihood_bound,
                              bool logits) {
  if (!ctx || count < 0 || (count && !items)) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = like_check(items, count, scale_bound, likelihood_bound, logits)) return rc;
  for (int i = 0; i < count; ++i) {
    const fgmm_like_grad_item &it = items[i];
    if (!it.dy && !it.dscales && !it.dmeans && !it.dweights) return fail(FGMM_ERR_INVALID, "item %d: every output is null", i);
    if (!it.g_like && !(fabs(it.g_bits) < (double)INFINITY)) return fail(FGMM_ERR_INVALID, "item %d: g_bits = %g is not finite", i, it.g_bits);
  }
  return latent_call(ctx, stream, items, count, [&](dev::Stream s) {
    return likelihood_backward_batch(ctx, s, items, count, round != 0, scale_bound, likelihood_bound, logits);
  });
}

} // namespace

extern "C" {

int fgmm_gmc_likelihood_batch(fgmm_ctx *ctx, void *stream, fgmm_like_item *items, int count, int round, float scale_bound, float likelihood_bound) {
  return likelihood_entry(ctx, stream, items, count, round, scale_bound, likelihood_bound, false);
}

int fgmm_gmc_likelihood_backward_batch(fgmm_ctx *ctx, void *stream, fgmm_like_grad_item *items, int count, int round, float scale_bound,
                                       float likelihood_bound) {
  return likelihood_backward_entry(ctx, stream, items, count, round, scale_bound, likelihood_bound, false);
}

int fgmm_gmc_likelihood_logits_batch(fgmm_ctx *ctx, void *stream, fgmm_like_item *items, int count, int round, float scale_bound,
                                     float likelihood_bound) {
  return likelihood_entry(ctx, stream, items, count, round, scale_bound, likelihood_bound, true);
}

int fgmm_gmc_likelihood_logits_backward_batch(fgmm_ctx *ctx, void *stream, fgmm_like_grad_item *items, int count, int round, float scale_bound,
                                              float likelihood_bound) {
  return likelihood_backward_entry(ctx, stream, items, count, round, scale_bound, likelihood_bound, true);
}

} // extern "C"
