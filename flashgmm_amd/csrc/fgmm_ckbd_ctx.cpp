// fgmm_ckbd_ctx.cpp — the checkerboard context convolution's entry points (include/flashgmm_amd.h section 5b) over fgmm_ckbd_ctx.hip: a
// handle that owns the packed weights (immutable once made, like a parameter head's), and a STREAM-ORDERED apply - validation, one
// launch, no workspace, no lock, no wait (a FGMM_CKBD_CTX_BF16X6 handle, over fgmm_ckbd_ctx16.hip: both packings, and an apply with
// the caller's workspace - the split, the bf16x6 kernel, the exact kernel for the items outside the domain); and section 5c over fgmm_ckbd_ctx_grad.hip: the same with caller-owned packed weights (a
// training step repacks every time), the transposed packing the data gradient runs on, and the weight and bias gradients.  A file of
// its own: the host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

struct fgmm_ckbd_context {
  int device = 0;
  int M = 0, c_out = 0;
  float *packed = nullptr;  // [wp | bp]
  void *packed16 = nullptr; // FGMM_CKBD_CTX_BF16X6: the three bf16 parts of the weights (fgmm_ckbd_ctx16.hip) - the handle holds both packings
};

extern "C" {

int fgmm_ckbd_ctx_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int c_out, fgmm_ckbd_context **out) {
  return fgmm_ckbd_ctx_create_ex(ctx, stream, weight, bias, M, c_out, 0, out);
}

int fgmm_ckbd_ctx_create_ex(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int M, int c_out, int flags, fgmm_ckbd_context **out) {
  if (!out) return fail(FGMM_ERR_INVALID, "out == NULL");
  *out = nullptr;
  if (!ctx || !weight || M <= 0 || c_out <= 0 || M > (1 << 20) || c_out > (1 << 20)) return fail(FGMM_ERR_INVALID, "context convolution: bad argument");
  if (flags & ~FGMM_CKBD_CTX_BF16X6) return fail(FGMM_ERR_INVALID, "context convolution: unknown flags 0x%x", (unsigned)flags);
  const bool b16 = (flags & FGMM_CKBD_CTX_BF16X6) != 0;
  if (b16 && ckbd_ctx16_mt(M) > 65535) return fail(FGMM_ERR_INVALID, "context convolution: bf16x6 takes at most %d input channels", 65535 * kHead16BK);
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  fgmm_ckbd_context *c = new (std::nothrow) fgmm_ckbd_context;
  if (!c) return fail(FGMM_ERR_NOMEM, "context convolution");
  c->device = ctx->device, c->M = M, c->c_out = c_out;
  const size_t floats = ckbd_ctx_packed_floats(M, c_out), bias_floats = (size_t)ckbd_ctx_row_tiles(c_out) * 32;
  void *p = nullptr;
  if (dev::malloc_device(&p, (floats + 4) * sizeof(float)) != 0) { // (+ the words the pack kernels flag a dropped tap and a weight outside the domain in)
    delete c;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed weights", floats * sizeof(float));
  }
  c->packed = static_cast<float *>(p);
  if (b16 && dev::malloc_device(&c->packed16, ckbd_ctx16_packed_bytes(M, c_out)) != 0) {
    (void)dev::free_device(p);
    delete c;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed bf16x6 weights", ckbd_ctx16_packed_bytes(M, c_out));
  }
  uint32_t *d_bad = reinterpret_cast<uint32_t *>(c->packed + floats); // [0]: a dropped tap is not zero; [1]: a kept tap outside the bf16x6 domain
  uint32_t bad[2] = {0, 0};
  int e = dev::memset_async(d_bad, 0, sizeof bad, (dev::Stream)stream);
  if (!e) e = launch_ckbd_ctx_pack(weight, bias, M, c_out, false, c->packed, c->packed + (floats - bias_floats), d_bad, stream);
  if (!e && b16) e = launch_ckbd_ctx16_pack(weight, M, c_out, c->packed16, d_bad + 1, stream);
  if (!e) e = dev::stream_sync((dev::Stream)stream); // (the caller may free or overwrite its weights on return)
  if (!e) e = dev::copy_sync(bad, d_bad, sizeof bad, dev::kD2H);
  if (e || bad[0] || bad[1]) {
    (void)dev::free_device(p);
    if (c->packed16) (void)dev::free_device(c->packed16);
    delete c;
    if (bad[0]) return fail(FGMM_ERR_INVALID, "context convolution: a dropped tap (kernel position (i, j) with i + j even) of the weights is not zero");
    if (bad[1]) return fail(FGMM_ERR_INVALID, "context convolution: a weight is outside the bf16x6 domain (finite, |w| < 0x1.FFp127)");
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
    if (c->packed16) (void)dev::free_device(c->packed16);
  }
  delete c;
}

// bf16x6: bytes of one item's split copy with its domain word (0: the sizes overflow), the whole workspace being n of them
static size_t ckbd_ctx16_item_bytes(int M, int n, int64_t hw) {
  const int64_t per_pos = (int64_t)ckbd_ctx16_mt(M) * 3 * kHead16BK * (int64_t)sizeof(uint16_t);
  if (n <= 0 || hw <= 0 || per_pos > (INT64_MAX / 4 - 64) / hw / n) return 0;
  return (size_t)(per_pos * hw) + kHead16FlagElems * sizeof(uint16_t);
}

// the checks the applies share, then the launches: one, or - c16, a bf16x6 handle - the split, the bf16x6 kernel and the exact kernel
// for the items the split flagged
static int ckbd_ctx_run(fgmm_ctx *ctx, void *stream, const float *packed, int M, int c_out, const float *anchors, float *out, int n, int64_t h, int64_t w,
                        int anchor_odd, const fgmm_ckbd_context *c16 = nullptr, void *workspace = nullptr, size_t workspace_bytes = 0) {
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
  size_t item_bytes = 0;
  if (c16) {
    item_bytes = ckbd_ctx16_item_bytes(M, n, hw);
    if (!item_bytes) return fail(FGMM_ERR_INVALID, "context convolution: n * channels * h * w/2 overflows");
    const size_t need = item_bytes * (size_t)n;
    if (!workspace || workspace_bytes < need)
      return fail(FGMM_ERR_INVALID, "context convolution: a workspace of %zu bytes, %zu needed (fgmm_ckbd_ctx_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(FGMM_ERR_INVALID, "context convolution: the workspace (%zu bytes needed) is not aligned to 16 bytes", need);
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  CkbdCtxArgs a;
  memset(&a, 0, sizeof a);
  const int mt = (M + kCkbdCtxBK - 1) / kCkbdCtxBK;
  a.anchors = anchors, a.out = out;
  a.wp = packed, a.bp = packed + (ckbd_ctx_packed_floats(M, c_out) - (size_t)ckbd_ctx_row_tiles(c_out) * 32);
  a.M = M, a.c_out = c_out, a.h = (int32_t)h, a.w2 = (int32_t)w2, a.odd = anchor_odd;
  a.mt = mt, a.n_kt = kCkbdCtxTaps * mt, a.pt = (int32_t)pt;
  if (c16) {
    const int64_t xs_stride = (int64_t)(item_bytes / sizeof(uint16_t));
    for (int i0 = 0; i0 < n; i0 += 65535) // (a grid's third dimension)
      LAUNCH_TRY(launch_head16_split(anchors + (int64_t)i0 * M * hw, static_cast<uint16_t *>(workspace) + i0 * xs_stride, hw, M, std::min(n - i0, 65535), (int64_t)M * hw,
                                     xs_stride, stream));
    CkbdCtx16Args b;
    memset(&b, 0, sizeof b);
    b.xs = static_cast<const uint16_t *>(workspace), b.xs_stride = xs_stride, b.out = out, b.wp16 = c16->packed16, b.bp = a.bp;
    b.M = M, b.c_out = c_out, b.h = a.h, b.w2 = a.w2, b.odd = anchor_odd;
    b.mt = ckbd_ctx16_mt(M), b.n_kt = kCkbdCtxTaps * b.mt, b.pt = a.pt;
    LAUNCH_TRY(launch_ckbd_ctx16(b, n, stream));
    a.only = head16_oob_word(workspace, M, hw), a.only_stride = xs_stride / 2; // (in 32-bit words)
  }
  LAUNCH_TRY(launch_ckbd_ctx(a, n, stream));
  return FGMM_OK;
}

int fgmm_ckbd_ctx_apply(fgmm_ctx *ctx, void *stream, const fgmm_ckbd_context *c, const float *anchors, float *out, int n, int64_t h, int64_t w,
                        int anchor_odd) {
  if (!ctx || !c) return fail(FGMM_ERR_INVALID, "context convolution: bad argument (n >= 0, h >= 1, w even and >= 2)");
  if (n >= 0 && h >= 1 && w >= 2 && !(w & 1) && !(anchor_odd & ~1) && c->device != ctx->device)
    return fail(FGMM_ERR_INVALID, "context convolution: made for device %d, context on %d", c->device, ctx->device);
  if (c->packed16) return fail(FGMM_ERR_INVALID, "context convolution: a bf16x6 handle needs a workspace: call fgmm_ckbd_ctx_apply_ws");
  return ckbd_ctx_run(ctx, stream, c->packed, c->M, c->c_out, anchors, out, n, h, w, anchor_odd);
}

size_t fgmm_ckbd_ctx_workspace_bytes(const fgmm_ckbd_context *c, int n, int64_t h, int64_t w) {
  if (!c || !c->packed16 || n <= 0 || h < 1 || w < 2 || (w & 1) || h > (INT32_MAX - 256) / (w / 2)) return 0;
  return ckbd_ctx16_item_bytes(c->M, n, h * (w / 2)) * (size_t)n;
}

int fgmm_ckbd_ctx_apply_ws(fgmm_ctx *ctx, void *stream, const fgmm_ckbd_context *c, const float *anchors, float *out, int n, int64_t h, int64_t w,
                           int anchor_odd, void *workspace, size_t workspace_bytes) {
  if (c && !c->packed16) return fgmm_ckbd_ctx_apply(ctx, stream, c, anchors, out, n, h, w, anchor_odd);
  if (!ctx || !c) return fail(FGMM_ERR_INVALID, "context convolution: bad argument (n >= 0, h >= 1, w even and >= 2)");
  if (n >= 0 && h >= 1 && w >= 2 && !(w & 1) && !(anchor_odd & ~1) && c->device != ctx->device)
    return fail(FGMM_ERR_INVALID, "context convolution: made for device %d, context on %d", c->device, ctx->device);
  return ckbd_ctx_run(ctx, stream, c->packed, c->M, c->c_out, anchors, out, n, h, w, anchor_odd, c, workspace, workspace_bytes);
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
