// fgmm_ckbd_ctx.cpp — the checkerboard context convolution's entry points (include/flashgmm_amd.h section 5b) over fgmm_ckbd_ctx.hip: a
// handle that owns the packed weights (immutable once made, like a parameter head's), and a STREAM-ORDERED apply - validation, one
// launch, no workspace, no lock, no wait; and section 5c over fgmm_ckbd_ctx_grad.hip: the same with caller-owned packed weights (a
// training step repacks every time), the transposed packing the data gradient runs on, and the weight and bias gradients.  A file of
// its own: the host sources that build against the fake device reference no launcher of these.
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
  if (!e) e = launch_ckbd_ctx_pack(weight, bias, M, c_out, false, c->packed, c->packed + (floats - bias_floats), d_bad, stream);
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

// the checks apply and apply_packed share, then the one launch
static int ckbd_ctx_run(fgmm_ctx *ctx, void *stream, const float *packed, int M, int c_out, const float *anchors, float *out, int n, int64_t h, int64_t w,
                        int anchor_odd) {
  if (n < 0 || h < 1 || w < 2 || (w & 1) || (anchor_odd & ~1))
    return fail(FGMM_ERR_INVALID, "context convolution: bad argument (n >= 0, h >= 1, w even and >= 2)");
  if (n == 0) return FGMM_OK;
  if (!anchors || !out) return fail(FGMM_ERR_INVALID, "context convolution: null tensor");
  if ((reinterpret_cast<uintptr_t>(anchors) | reinterpret_cast<uintptr_t>(out)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "context convolution: misaligned tensor");
  // positions of an item are indexed in 32 bits, blocks in 30 (head_launch's limit)
  const int64_t w2 = w / 2;
  if (h > (INT32_MAX - 256) / w2) return fail(FGMM_ERR_INVALID, "context convolution: h * w/2 = %lld x %lld positions exceed 2^31", (long long)h, (long long)w2);
  const int64_t hw = h * w2, pt = (hw + 127) / 128, n_rt = (c_out + 31) / 32; // (at most a block per row tile of 32)
  if (pt * n_rt > (1ll << 30) / n) return fail(FGMM_ERR_INVALID, "context convolution: %d x %lld x %lld workgroups exceed a grid", n, (long long)pt, (long long)n_rt);
  if (hw > INT64_MAX / 4 / n / std::max(M, c_out)) return fail(FGMM_ERR_INVALID, "context convolution: n * channels * h * w/2 overflows");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  CkbdCtxArgs a;
  memset(&a, 0, sizeof a);
  const int mt = (M + kCkbdCtxBK - 1) / kCkbdCtxBK;
  a.anchors = anchors, a.out = out;
  a.wp = packed, a.bp = packed + (ckbd_ctx_packed_floats(M, c_out) - (size_t)ckbd_ctx_row_tiles(c_out) * 32);
  a.M = M, a.c_out = c_out, a.h = (int32_t)h, a.w2 = (int32_t)w2, a.odd = anchor_odd;
  a.mt = mt, a.n_kt = kCkbdCtxTaps * mt, a.pt = (int32_t)pt;
  LAUNCH_TRY(launch_ckbd_ctx(a, n, stream));
  return FGMM_OK;
}

int fgmm_ckbd_ctx_apply(fgmm_ctx *ctx, void *stream, const fgmm_ckbd_context *c, const float *anchors, float *out, int n, int64_t h, int64_t w,
                        int anchor_odd) {
  if (!ctx || !c) return fail(FGMM_ERR_INVALID, "context convolution: bad argument (n >= 0, h >= 1, w even and >= 2)");
  if (n >= 0 && h >= 1 && w >= 2 && !(w & 1) && !(anchor_odd & ~1) && c->device != ctx->device)
    return fail(FGMM_ERR_INVALID, "context convolution: made for device %d, context on %d", c->device, ctx->device);
  return ckbd_ctx_run(ctx, stream, c->packed, c->M, c->c_out, anchors, out, n, h, w, anchor_odd);
}

// ---- section 5c: caller-owned packed weights, and the gradients ---------------------------------------------------
static bool ckbd_sizes_ok(int M, int c_out) { return M > 0 && c_out > 0 && M <= (1 << 20) && c_out <= (1 << 20); }

size_t fgmm_ckbd_ctx_packed_floats(int M, int c_out) { return ckbd_sizes_ok(M, c_out) ? ckbd_ctx_packed_floats(M, c_out) : 0; }

int fgmm_ckbd_ctx_pack(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int c_out, int transposed, float *packed) {
  if (!ctx || !weight || !packed || !ckbd_sizes_ok(M, c_out) || (transposed & ~1) || (transposed && bias))
    return fail(FGMM_ERR_INVALID, "context convolution: bad argument to pack (null tensor, sizes, a bias with the transposed form)");
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(packed)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "context convolution: misaligned tensor");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  const int pm = transposed ? c_out : M, pc = transposed ? M : c_out; // the packed convolution's sizes
  LAUNCH_TRY(launch_ckbd_ctx_pack(weight, bias, M, c_out, transposed != 0, packed,
                                  packed + (ckbd_ctx_packed_floats(pm, pc) - (size_t)ckbd_ctx_row_tiles(pc) * 32), nullptr, stream));
  return FGMM_OK;
}

int fgmm_ckbd_ctx_apply_packed(fgmm_ctx *ctx, void *stream, const float *packed, int M, int c_out, const float *anchors, float *out, int n, int64_t h,
                               int64_t w, int anchor_odd) {
  if (!ctx || !ckbd_sizes_ok(M, c_out)) return fail(FGMM_ERR_INVALID, "context convolution: bad argument (context, channel counts)");
  if (n > 0 && (!packed || reinterpret_cast<uintptr_t>(packed) % sizeof(float))) return fail(FGMM_ERR_INVALID, "context convolution: null or misaligned packed weights");
  return ckbd_ctx_run(ctx, stream, packed, M, c_out, anchors, out, n, h, w, anchor_odd);
}

// the shared validation of the two wgrad entry points: -> P = n * h * w/2 (0: nothing to do), or -1 with the error set
static int64_t ckbd_wgrad_positions(int M, int c_out, int n, int64_t h, int64_t w) {
  if (!ckbd_sizes_ok(M, c_out) || n < 0 || h < 1 || w < 2 || (w & 1)) {
    fail(FGMM_ERR_INVALID, "context convolution gradient: bad argument (channel counts, n >= 0, h >= 1, w even and >= 2)");
    return -1;
  }
  const int64_t w2 = w / 2;
  if (h > (INT32_MAX - 256) / w2 || (n > 0 && h * w2 > (INT32_MAX - 256) / n)) {
    fail(FGMM_ERR_INVALID, "context convolution gradient: n * h * w/2 = %d x %lld x %lld positions exceed 2^31", n, (long long)h, (long long)w2);
    return -1;
  }
  if (n > 0 && h * w2 > INT64_MAX / 4 / n / std::max(M, c_out)) {
    fail(FGMM_ERR_INVALID, "context convolution gradient: n * channels * h * w/2 overflows");
    return -1;
  }
  return (int64_t)n * h * w2;
}

size_t fgmm_ckbd_ctx_wgrad_workspace(int M, int c_out, int n, int64_t h, int64_t w) {
  const int64_t P = ckbd_wgrad_positions(M, c_out, n, h, w);
  if (P <= 0) return 0;
  return (size_t)ckbd_wgrad_slices(P).S * (size_t)c_out * (size_t)ckbd_wgrad_cols(M) * sizeof(float);
}

int fgmm_ckbd_ctx_wgrad(fgmm_ctx *ctx, void *stream, const float *anchors, const float *g, int M, int c_out, int n, int64_t h, int64_t w, int anchor_odd,
                        float *dweight, float *dbias, void *workspace, size_t workspace_bytes) {
  if (!ctx || (anchor_odd & ~1)) return fail(FGMM_ERR_INVALID, "context convolution gradient: bad argument (context, anchor_odd)");
  const int64_t P = ckbd_wgrad_positions(M, c_out, n, h, w);
  if (P < 0) return FGMM_ERR_INVALID;
  if (n == 0) return FGMM_OK;
  if (!dweight && !dbias) return fail(FGMM_ERR_INVALID, "context convolution gradient: neither dweight nor dbias");
  if (!g || (dweight && !anchors)) return fail(FGMM_ERR_INVALID, "context convolution gradient: null tensor");
  if ((reinterpret_cast<uintptr_t>(anchors) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dweight) | reinterpret_cast<uintptr_t>(dbias)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "context convolution gradient: misaligned tensor");
  const CkbdWgradSlices sl = ckbd_wgrad_slices(P);
  const size_t need = (size_t)sl.S * (size_t)c_out * (size_t)ckbd_wgrad_cols(M) * sizeof(float);
  if (!workspace || workspace_bytes < need) return fail(FGMM_ERR_INVALID, "context convolution gradient: a workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, need);
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(FGMM_ERR_INVALID, "context convolution gradient: the workspace is not aligned to 16 bytes");
  const int64_t col_groups = ((int64_t)kCkbdCtxTaps * ((M + kCkbdCtxBK - 1) / kCkbdCtxBK) + 4) / 4, n_rt = (c_out + 31) / 32; // (at most a block per row tile)
  if (sl.S * col_groups * n_rt > (1ll << 30))
    return fail(FGMM_ERR_INVALID, "context convolution gradient: %lld x %lld x %lld workgroups exceed a grid", (long long)sl.S, (long long)col_groups, (long long)n_rt);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  CkbdWgradArgs a;
  memset(&a, 0, sizeof a);
  const int mt = (M + kCkbdCtxBK - 1) / kCkbdCtxBK;
  a.anchors = anchors, a.g = g, a.partial = static_cast<float *>(workspace);
  a.M = M, a.c_out = c_out, a.h = (int32_t)h, a.w2 = (int32_t)(w / 2), a.odd = anchor_odd, a.mt = mt;
  a.col0 = dweight ? 0 : kCkbdCtxTaps * mt, a.n_col = (dweight ? kCkbdCtxTaps * mt : 0) + (dbias ? 1 : 0); // the bias' column tile is the last
  a.P = (int32_t)P, a.L = (int32_t)sl.L, a.S = (int32_t)sl.S;
  LAUNCH_TRY(launch_ckbd_wgrad(a, stream));
  LAUNCH_TRY(launch_ckbd_wgrad_finish(a.partial, M, c_out, a.S, dweight, dbias, stream));
  return FGMM_OK;
}

} // extern "C"
