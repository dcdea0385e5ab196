// fgmm_like.cpp — the entropy model's forward(): the likelihood of a batch of latents, its rate, and the gradients of either
// (include/flashgmm_amd.h section 3g, and 3h: the same on the parameter head's logits, the softmax over K and its derivative in the
// kernels).  Orchestration over fgmm_like.hip behind two entry points per section, in the shell of the pricing calls
// (fgmm_ctx.h: latent_call, check_latent_items) but without their census front half: every channel is evaluated.  Per call, whatever
// the number of items: one upload of descriptors, one memset of the sums, one launch, one small copy back.  A file of its own: the
// host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

namespace {

// the EncDesc of an item of these calls: its latent and planes, no census (chan_list null), no table
void like_desc(EncDesc &d, const float *y, const fgmm_params &p, int M, int64_t hw) {
  memset(&d, 0, sizeof d);
  d.y = y;
  d.scales = p.scales, d.means = p.means, d.weights = p.weights;
  d.stride_k = p.stride_k, d.stride_c = p.stride_c, d.stride_p = 1;
  d.hw = hw;
  d.M = M;
  d.seg_b[0] = d.seg_b[1] = d.seg_b[2] = INT32_MAX;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// positions per lane (8, two-byte planes only; 4; 1) and the grid every item of the batch allows
struct LikeShape {
  int M_max = 0, vec = 1;
  int64_t hw_max = 0, n_max = 0;
  bool linear = true, vec4 = true, vec8 = true;
  void item(const EncDesc &d, bool two_byte, std::initializer_list<const void *> others) {
    bool ok4 = true, ok16 = true;
    for (const void *o : others) ok4 = ok4 && enc_vec4_ok(d, o, two_byte), ok16 = ok16 && aligned16(o);
    vec4 = vec4 && ok4;
    vec8 = vec8 && ok4 && ok16 && two_byte && (d.hw & 7) == 0 && (d.stride_c & 7) == 0 && (d.stride_k & 7) == 0 && aligned16(d.scales) &&
           aligned16(d.means) && aligned16(d.weights);
    M_max = std::max(M_max, d.M);
    hw_max = std::max(hw_max, d.hw);
    n_max = std::max(n_max, (int64_t)d.M * d.hw);
  }
  void done(const EncDesc *hd, int count, int vec_cap) {
    vec = vec4 ? (vec8 && vec_cap >= 8 ? 8 : 4) : 1;
    auto fills = [&](int v) { // every wave of the linear grid full at v positions per lane
      for (int i = 0; i < count; ++i)
        if (hd[i].hw % (64 * v)) return false;
      return true;
    };
    // 8 per lane only where that keeps the linear grid: a 768-position Kodak plane fills 96 of the 256 lanes of its tiled block at 8 per
    // lane, and every wave of the linear grid at 4
    if (vec == 8 && !fills(8) && fills(4)) vec = 4;
    linear = fills(vec);
  }
};

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
