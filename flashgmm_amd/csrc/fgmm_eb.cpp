// fgmm_eb.cpp — the entropy bottleneck's forward(): the likelihood of the hyper-latent under its factorized density, its rate, and the
// gradients of either (include/flashgmm_amd.h section 3j).  Orchestration over fgmm_eb.hip behind two entry points, in the shell of the
// likelihood calls (fgmm_ctx.h: latent_call).  Forward: one memset of the items' sums, one launch, one small copy back.  Backward: at most
// one small upload (the items' g_bits), two launches - the partial rows [C][S][59] live in the context's workspace.  update() (section
// 3k): the quantile search, one launch and nothing else; the tables, one launch, the rows back and the integer quantiser.  A file of its own:
// the host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

namespace {

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; } // (null counts as aligned)

template <class Call> int eb_check(const Call *call, int mode, float lb) {
  if (!call->x || !call->theta || !call->med) return fail(FGMM_ERR_INVALID, "null x, theta or med");
  if (call->B < 1 || call->C < 1 || call->hw < 1)
    return fail(FGMM_ERR_INVALID, "B = %d, C = %d, hw = %lld: each must be at least 1", call->B, call->C, (long long)call->hw);
  if (mode != 0 && mode != 1) return fail(FGMM_ERR_INVALID, "mode = %d: 0 (the values as they are) or 1 (dequantize)", mode);
  if (!(lb >= 0.0f) || !(lb < INFINITY)) return fail(FGMM_ERR_INVALID, "likelihood_bound = %g: must be finite and >= 0", (double)lb);
  if (call->hw > INT64_MAX / call->B / call->C) return fail(FGMM_ERR_INVALID, "B * C * hw overflows");
  const int64_t S = ((int64_t)call->B * call->hw + FGMM_EB_SLICE - 1) / FGMM_EB_SLICE;
  if (S * call->C > 0x7FFFFFFFll) return fail(FGMM_ERR_UNSUPPORTED, "C * ceil(B * hw / %d) = %lld workgroups exceed a grid", FGMM_EB_SLICE, (long long)(S * call->C));
  return FGMM_OK;
}

template <class Call> EbArgs eb_args(const Call &c, int mode, float lb) {
  EbArgs a;
  memset(&a, 0, sizeof a);
  a.x = c.x, a.theta = c.theta, a.med = c.med;
  a.hw = c.hw, a.n = (int64_t)c.B * c.hw;
  a.B = c.B, a.C = c.C, a.S = (int32_t)((a.n + FGMM_EB_SLICE - 1) / FGMM_EB_SLICE), a.mode = mode;
  a.lb = lb;
  return a;
}

int eb_forward(fgmm_ctx *ctx, dev::Stream stream, fgmm_eb_call *call, int mode, float lb) {
  Arena ar;
  const size_t o_sums = ar.take(2 * sizeof(uint64_t) * (size_t)call->B), end = ar.off;
  int rc;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(end)) || (rc = ctx->ensure_events(1))) return rc;
  EbArgs a = eb_args(*call, mode, lb);
  a.like = call->like_out, a.v = call->v_out;
  a.sums = ws<unsigned long long>(ctx->d_ws, o_sums);
  const int vec = (call->hw & 3) == 0 && aligned16(call->x) && aligned16(call->like_out) && aligned16(call->v_out) ? 4 : 1;
  DEV_TRY(dev::memset_async(ctx->d_ws + o_sums, 0, end - o_sums, stream));
  LAUNCH_TRY(launch_eb(a, vec, stream));
  DEV_TRY(dev::copy_async(ctx->h_ws + o_sums, ctx->d_ws + o_sums, end - o_sums, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  const uint64_t *sums = ws<const uint64_t>(ctx->h_ws, o_sums);
  for (int b = 0; b < call->B; ++b) {
    if (call->bits_q) call->bits_q[b] = (int64_t)sums[2 * b];
    if (call->n_nonfinite) call->n_nonfinite[b] = (int64_t)sums[2 * b + 1];
  }
  call->status = FGMM_OK;
  return FGMM_OK;
}

int eb_backward(fgmm_ctx *ctx, dev::Stream stream, fgmm_eb_grad_call *call, int mode, float lb) {
  EbArgs a = eb_args(*call, mode, lb);
  Arena ar;
  const size_t o_gbits = ar.take(sizeof(float) * (size_t)call->B), host_end = ar.off;
  const size_t o_rows = ar.take(sizeof(double) * (size_t)kEbRow * (size_t)a.S * (size_t)call->C), end = ar.off;
  int rc;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(host_end)) || (rc = ctx->ensure_events(1))) return rc;
  a.g_like = call->g_like, a.dx = call->dx;
  a.gbits = ws<const float>(ctx->d_ws, o_gbits);
  a.rows = ws<double>(ctx->d_ws, o_rows);
  if (!call->g_like) {
    float *h = ws<float>(ctx->h_ws, o_gbits);
    for (int b = 0; b < call->B; ++b) h[b] = (float)call->g_bits[b];
    DEV_TRY(dev::copy_async(ctx->d_ws + o_gbits, h, host_end - o_gbits, dev::kH2D, stream));
  }
  LAUNCH_TRY(launch_eb_bwd(a, stream));
  if (call->dtheta || call->dmed) LAUNCH_TRY(launch_eb_finish(call->theta, a.rows, call->dtheta, call->dmed, call->C, a.S, mode, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  call->status = FGMM_OK;
  return FGMM_OK;
}

// ---- section 3k: update() ------------------------------------------------------------------------------------------------------------
// the shell of latent_call for a call without items: the context's lock and device around `body(stream)`; a failure drains the stream
template <class Body> int eb_update_call(fgmm_ctx *ctx, void *stream, Body body) {
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const int rc = body((dev::Stream)stream);
  if (rc != FGMM_OK) (void)dev::stream_sync((dev::Stream)stream);
  return rc;
}

// One launch into the workspace, the rows and the lengths back, the integer quantiser per channel on the host; the caller's arrays are
// written last, once every channel has passed.
int eb_tables(fgmm_ctx *ctx, dev::Stream stream, const float *theta, const float *start, const int32_t *length, int C, int stride, float *pmf_out,
              int32_t *cdf_out, int32_t *failed) {
  Arena ar;
  const size_t n = (size_t)C * (size_t)stride;
  const size_t o_pmf = ar.take(sizeof(float) * n), o_len = ar.take(sizeof(int32_t) * (size_t)C), end = ar.off;
  int rc;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(end)) || (rc = ctx->ensure_events(1))) return rc;
  float *d_pmf = ws<float>(ctx->d_ws, o_pmf);
  LAUNCH_TRY(launch_eb_pmf(theta, start, length, C, stride, d_pmf, stream));
  DEV_TRY(dev::copy_async(ctx->h_ws + o_pmf, d_pmf, sizeof(float) * n, dev::kD2H, stream));
  DEV_TRY(dev::copy_async(ctx->h_ws + o_len, length, sizeof(int32_t) * (size_t)C, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  const float *pmf = ws<const float>(ctx->h_ws, o_pmf);
  const int32_t *len = ws<const int32_t>(ctx->h_ws, o_len);
  std::vector<int32_t> cdf((size_t)C * ((size_t)stride + 1), 0);
  for (int c = 0; c < C; ++c) {
    const float *row = pmf + (size_t)c * (size_t)stride;
    if (failed) *failed = c;
    if (len[c] < 1 || (int64_t)len[c] + 1 > stride) return fail(FGMM_ERR_INVALID, "channel %d: length = %d does not fit a row of %d entries with its tail", c, len[c], stride);
    for (int i = 0; i <= len[c]; ++i)
      if (!(row[i] >= 0.0f) || !(row[i] < INFINITY))
        return fail(FGMM_ERR_INVALID, "channel %d: the mass of entry %d of %d is %g", c, i, len[c] + 1, (double)row[i]);
    if (len[c] + 1 > 65536) return fail(FGMM_ERR_INVALID, "channel %d: %d symbols (its support and the tail) exceed 2^16 counts", c, len[c] + 1);
    if (pmf_to_quantized_cdf(row, len[c] + 1, 16, reinterpret_cast<uint32_t *>(cdf.data() + (size_t)c * ((size_t)stride + 1))) != FGMM_OK)
      return fail(FGMM_ERR_INVALID, "channel %d: every mass rounds to zero", c);
  }
  if (failed) *failed = -1;
  if (pmf_out) { // (the workspace is the next call's: the copy has completed before this one returns)
    DEV_TRY(dev::copy_async(pmf_out, d_pmf, sizeof(float) * n, dev::kD2D, stream));
    DEV_TRY(dev::event_record(ctx->events[0], stream));
    DEV_TRY(dev::event_sync(ctx->events[0]));
  }
  memcpy(cdf_out, cdf.data(), sizeof(int32_t) * cdf.size());
  return FGMM_OK;
}

} // namespace

extern "C" {

int fgmm_eb_quantiles(fgmm_ctx *ctx, void *stream, const float *theta, int C, const float *targets, float search_radius, float *q_out) {
  if (!ctx || !theta || !targets || !q_out) return fail(FGMM_ERR_INVALID, "null ctx, theta, targets or q_out");
  if (C < 1) return fail(FGMM_ERR_INVALID, "C = %d: must be at least 1", C);
  if (!(search_radius > 0.0f) || !(search_radius < INFINITY)) return fail(FGMM_ERR_INVALID, "search_radius = %g: must be finite and > 0", (double)search_radius);
  EbTargets t;
  for (int k = 0; k < 3; ++k) {
    if (targets[k] != targets[k]) return fail(FGMM_ERR_INVALID, "targets[%d] is NaN", k);
    t.t[k] = targets[k];
  }
  return eb_update_call(ctx, stream, [&](dev::Stream s) {
    LAUNCH_TRY(launch_eb_quantiles(theta, C, t, search_radius, q_out, s));
    return (int)FGMM_OK;
  });
}

int fgmm_eb_tables(fgmm_ctx *ctx, void *stream, const float *theta, const float *start, const int32_t *length, int C, int stride, float *pmf_out,
                   int32_t *cdf_out, int32_t *failed_channel_out) {
  if (!ctx || !theta || !start || !length || !cdf_out) return fail(FGMM_ERR_INVALID, "null ctx, theta, start, length or cdf_out");
  if (C < 1 || stride < 2) return fail(FGMM_ERR_INVALID, "C = %d, stride = %d: at least 1 channel and 2 entries (one mass and the tail)", C, stride);
  if ((int64_t)C * stride > 0x7FFFFFFFll) return fail(FGMM_ERR_INVALID, "C * stride = %lld exceeds 2^31 - 1", (long long)C * stride);
  if (failed_channel_out) *failed_channel_out = -1;
  return eb_update_call(ctx, stream, [&](dev::Stream s) { return eb_tables(ctx, s, theta, start, length, C, stride, pmf_out, cdf_out, failed_channel_out); });
}

int fgmm_eb_likelihood(fgmm_ctx *ctx, void *stream, fgmm_eb_call *call, int mode, float likelihood_bound) {
  if (!ctx || !call) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = eb_check(call, mode, likelihood_bound)) return rc;
  return latent_call(ctx, stream, call, 1, [&](dev::Stream s) { return eb_forward(ctx, s, call, mode, likelihood_bound); });
}

int fgmm_eb_likelihood_backward(fgmm_ctx *ctx, void *stream, fgmm_eb_grad_call *call, int mode, float likelihood_bound) {
  if (!ctx || !call) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = eb_check(call, mode, likelihood_bound)) return rc;
  if (!call->dx && !call->dtheta && !call->dmed) return fail(FGMM_ERR_INVALID, "every output is null");
  if (!call->g_like) {
    if (!call->g_bits) return fail(FGMM_ERR_INVALID, "neither g_like nor g_bits");
    for (int b = 0; b < call->B; ++b)
      if (!(fabs(call->g_bits[b]) < (double)INFINITY)) return fail(FGMM_ERR_INVALID, "g_bits[%d] = %g is not finite", b, call->g_bits[b]);
  }
  return latent_call(ctx, stream, call, 1, [&](dev::Stream s) { return eb_backward(ctx, s, call, mode, likelihood_bound); });
}

} // extern "C"
