// fgmm_ckbd_ctx.cpp — the checkerboard context convolution's entry points (include/flashgmm_amd.h section 5b) over fgmm_ckbd_ctx.hip: a
// handle that owns the packed weights (immutable once made, like a parameter head's), and a STREAM-ORDERED apply - validation, one
// launch, no workspace, no lock, no wait.  A file of its own: the host sources that build against the fake device reference no launcher
// of these.
#include "fgmm_ctx.h"

using namespace fgmm;

struct fgmm_ckbd_context {
  int device = 0;
  int M = 0, c_out = 0;
  float *packed = nullptr; // [wp | bp]
};

extern "C" {

int fgmm_ckbd_ctx_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int c_out, fgmm_ckbd_context **out) {
  if (!out) return fail(FGMM_ERR_INVALID, "out == NULL");
  *out = nullptr;
  if (!ctx || !weight || M <= 0 || c_out <= 0 || M > (1 << 20) || c_out > (1 << 20)) return fail(FGMM_ERR_INVALID, "context convolution: bad argument");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  fgmm_ckbd_context *c = new (std::nothrow) fgmm_ckbd_context;
  if (!c) return fail(FGMM_ERR_NOMEM, "context convolution");
  c->device = ctx->device, c->M = M, c->c_out = c_out;
  const size_t floats = ckbd_ctx_packed_floats(M, c_out), bias_floats = (size_t)ckbd_ctx_row_tiles(c_out) * 32;
  void *p = nullptr;
  if (dev::malloc_device(&p, (floats + 4) * sizeof(float)) != 0) { // (+ the word the pack kernel flags a dropped tap in)
    delete c;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed weights", floats * sizeof(float));
  }
  c->packed = static_cast<float *>(p);
  uint32_t *d_bad = reinterpret_cast<uint32_t *>(c->packed + floats);
  uint32_t bad = 0;
  int e = dev::memset_async(d_bad, 0, sizeof(uint32_t), (dev::Stream)stream);
  if (!e) e = launch_ckbd_ctx_pack(weight, bias, M, c_out, c->packed, c->packed + (floats - bias_floats), d_bad, stream);
  if (!e) e = dev::stream_sync((dev::Stream)stream); // (the caller may free or overwrite its weights on return)
  if (!e) e = dev::copy_sync(&bad, d_bad, sizeof(uint32_t), dev::kD2H);
  if (e || bad) {
    (void)dev::free_device(p);
    delete c;
    if (bad) return fail(FGMM_ERR_INVALID, "context convolution: a dropped tap (kernel position (i, j) with i + j even) of the weights is not zero");
    return fail(FGMM_ERR_HIP, "packing the context convolution's weights: %s", dev::error_string(e));
  }
  *out = c;
  return FGMM_OK;
}

void fgmm_ckbd_ctx_destroy(fgmm_ckbd_context *c) {
  if (!c) return;
  {
    DeviceGuard g(c->device);
    (void)dev::free_device(c->packed);
  }
  delete c;
}

int fgmm_ckbd_ctx_apply(fgmm_ctx *ctx, void *stream, const fgmm_ckbd_context *c, const float *anchors, float *out, int n, int64_t h, int64_t w,
                        int anchor_odd) {
  if (!ctx || !c || n < 0 || h < 1 || w < 2 || (w & 1) || (anchor_odd & ~1))
    return fail(FGMM_ERR_INVALID, "context convolution: bad argument (n >= 0, h >= 1, w even and >= 2)");
  if (c->device != ctx->device) return fail(FGMM_ERR_INVALID, "context convolution: made for device %d, context on %d", c->device, ctx->device);
  if (n == 0) return FGMM_OK;
  if (!anchors || !out) return fail(FGMM_ERR_INVALID, "context convolution: null tensor");
  if ((reinterpret_cast<uintptr_t>(anchors) | reinterpret_cast<uintptr_t>(out)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "context convolution: misaligned tensor");
  // positions of an item are indexed in 32 bits, blocks in 30 (head_launch's limit)
  const int64_t w2 = w / 2;
  if (h > (INT32_MAX - 256) / w2) return fail(FGMM_ERR_INVALID, "context convolution: h * w/2 = %lld x %lld positions exceed 2^31", (long long)h, (long long)w2);
  const int64_t hw = h * w2, pt = (hw + 127) / 128, n_rt = (c->c_out + 31) / 32; // (at most a block per row tile of 32)
  if (pt * n_rt > (1ll << 30) / n) return fail(FGMM_ERR_INVALID, "context convolution: %d x %lld x %lld workgroups exceed a grid", n, (long long)pt, (long long)n_rt);
  if (hw > INT64_MAX / 4 / n / std::max(c->M, c->c_out)) return fail(FGMM_ERR_INVALID, "context convolution: n * channels * h * w/2 overflows");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  CkbdCtxArgs a;
  memset(&a, 0, sizeof a);
  const int mt = (c->M + kCkbdCtxBK - 1) / kCkbdCtxBK;
  a.anchors = anchors, a.out = out;
  a.wp = c->packed, a.bp = c->packed + (ckbd_ctx_packed_floats(c->M, c->c_out) - (size_t)ckbd_ctx_row_tiles(c->c_out) * 32);
  a.M = c->M, a.c_out = c->c_out, a.h = (int32_t)h, a.w2 = (int32_t)w2, a.odd = anchor_odd;
  a.mt = mt, a.n_kt = kCkbdCtxTaps * mt, a.pt = (int32_t)pt;
  LAUNCH_TRY(launch_ckbd_ctx(a, n, stream));
  return FGMM_OK;
}

} // extern "C"
