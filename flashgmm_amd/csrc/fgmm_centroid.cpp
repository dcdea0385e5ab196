// fgmm_centroid.cpp — centroid reconstruction of a batch of decoded latents (include/flashgmm_amd.h section 3i).  Orchestration over
// fgmm_centroid.hip behind one entry point, in the shell of the likelihood calls (fgmm_ctx.h: latent_call, check_latent_items, like_desc,
// LikeShape - the forward's load width and grid, decided the same way).  Per call, whatever the number of items: one upload of
// descriptors, one memset of the counts, one launch, one copy back of 8 bytes per item, the call's one wait.  A file of its own: the host
// sources that build against the fake device reference no launcher of this.
#include "fgmm_ctx.h"

using namespace fgmm;

namespace {

int centroid_check(const fgmm_centroid_item *items, int count, float scale_bound, float p_min) {
  if (!(scale_bound > 0.0f) || !(scale_bound < INFINITY)) return fail(FGMM_ERR_INVALID, "scale_bound = %g: must be positive and finite", (double)scale_bound);
  if (!(p_min > 0.0f) || !(p_min < INFINITY)) return fail(FGMM_ERR_INVALID, "p_min = %g: must be positive and finite", (double)p_min);
  if (int rc = check_latent_items(latent_in(items, count))) return rc;
  for (int i = 0; i < count; ++i) {
    if (items[i].params.flags != items[0].params.flags) // one call is one form: the planes of weights all hold weights, or all logits
      return fail(FGMM_ERR_INVALID, "item %d: fgmm_params.flags %d differ from item 0's %d", i, items[i].params.flags, items[0].params.flags);
    if (!items[i].y || !items[i].rec) return fail(FGMM_ERR_INVALID, "item %d: null y or rec", i);
  }
  return FGMM_OK;
}

int centroid_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_centroid_item *items, int count, float sb, float p_min) {
  Arena ar;
  const size_t o_descs = ar.take(sizeof(EncDesc) * (size_t)count), o_call = ar.take(sizeof(CentroidDesc) * (size_t)count);
  const size_t o_kept = ar.take(sizeof(uint64_t) * (size_t)count), end = ar.off;
  int rc;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(end)) || (rc = ctx->ensure_events(1))) return rc;
  EncDesc *hd = ws<EncDesc>(ctx->h_ws, o_descs);
  CentroidDesc *hc = ws<CentroidDesc>(ctx->h_ws, o_call);
  LikeShape sh;
  const int planes = items[0].params.dtype;
  const bool logits = items[0].params.flags == FGMM_PARAMS_LOGITS;
  for (int i = 0; i < count; ++i) {
    const fgmm_centroid_item &it = items[i];
    like_desc(hd[i], it.y, it.params, it.M, it.hw);
    hc[i] = CentroidDesc{it.rec, ws<unsigned long long>(ctx->d_ws, o_kept) + i};
    sh.item(hd[i], planes_two_byte(planes), {it.rec});
  }
  sh.done(hd, count, 8);
  DEV_TRY(dev::copy_async(ctx->d_ws + o_descs, hd, o_kept - o_descs, dev::kH2D, stream)); // (both descriptor arrays: one copy)
  DEV_TRY(dev::memset_async(ctx->d_ws + o_kept, 0, end - o_kept, stream));
  LAUNCH_TRY(launch_centroid(ws<const EncDesc>(ctx->d_ws, o_descs), ws<const CentroidDesc>(ctx->d_ws, o_call), sb, p_min, count, sh.M_max, sh.hw_max,
                             sh.n_max, sh.linear, sh.vec, planes, logits, stream));
  DEV_TRY(dev::copy_async(ctx->h_ws + o_kept, ctx->d_ws + o_kept, end - o_kept, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  const uint64_t *kept = ws<const uint64_t>(ctx->h_ws, o_kept);
  for (int i = 0; i < count; ++i) {
    items[i].n_kept = (int64_t)kept[i];
    items[i].status = FGMM_OK;
  }
  return FGMM_OK;
}

} // namespace

extern "C" int fgmm_gmc_centroid_batch(fgmm_ctx *ctx, void *stream, fgmm_centroid_item *items, int count, float scale_bound, float p_min) {
  if (!ctx || count < 0 || (count && !items)) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = centroid_check(items, count, scale_bound, p_min)) return rc;
  return latent_call(ctx, stream, items, count, [&](dev::Stream s) { return centroid_batch(ctx, s, items, count, scale_bound, p_min); });
}
