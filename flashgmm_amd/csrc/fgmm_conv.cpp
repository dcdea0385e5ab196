// fgmm_conv.cpp — the entry points of the dense 3x3 / 5x5 convolution layers (include/flashgmm_amd.h section 5d) over fgmm_conv.hip: a
// handle that owns one layer's packed weights (immutable once made, like a hidden layer's) and a STREAM-ORDERED apply - validation, one
// launch, no workspace, no lock, no wait.  A file of its own: the host sources that build against the fake device reference no launcher
// of these.  The transposed layers of section 5e (fgmm_conv_create_transposed) are the same handle: stride 1 on fgmm_conv.hip's kernel
// over the flipped pack, stride 2 on fgmm_deconv.hip; apply dispatches on the handle.  A FGMM_CONV_BF16X6 handle (fgmm_conv_create_ex, over
// fgmm_conv16.hip) owns both packings, and its apply takes the caller's workspace: the split of the input, the bf16x6 kernel, the exact
// kernel for the items outside the domain.
#include "fgmm_ctx.h"

using namespace fgmm;

struct fgmm_conv {
  int device = 0;
  int c_out = 0, c_in = 0, k = 0, act = 0, shuffle = 1;
  int stride = 0; // 0: a Conv2d layer (section 5d); 1 | 2: a ConvTranspose2d layer of that stride (section 5e)
  float slope = 0.0f;
  float *packed = nullptr; // [wp | bp]
  void *packed16 = nullptr; // FGMM_CONV_BF16X6: the three bf16 parts of the weights (fgmm_conv16.hip) - the handle holds both packings
};

// what every call that names a layer refuses of its sizes, activation and store: 0, or FGMM_ERR_INVALID with the message set
static int conv_layer_bad(int c_out, int c_in, int k, int act, float slope, int shuffle) {
  if (k != 3 && k != 5) return fail(FGMM_ERR_INVALID, "convolution: k = %d (3 or 5)", k);
  if (c_out < 1 || c_in < 1 || c_out > (1 << 20) || c_in > (1 << 20))
    return fail(FGMM_ERR_INVALID, "convolution: c_out = %d, c_in = %d (each from 1 to 2^20)", c_out, c_in);
  if (act != FGMM_ACT_NONE && act != FGMM_ACT_LEAKY && act != FGMM_ACT_RELU) return fail(FGMM_ERR_INVALID, "convolution: unknown activation %d", act);
  if (!std::isfinite(slope)) return fail(FGMM_ERR_INVALID, "convolution: the slope is not finite");
  if (shuffle != 1 && shuffle != 2) return fail(FGMM_ERR_INVALID, "convolution: shuffle = %d (1 or 2)", shuffle);
  if (shuffle == 2 && c_out % 4) return fail(FGMM_ERR_INVALID, "convolution: shuffle 2 needs c_out = %d to be a multiple of 4", c_out);
  return 0;
}

// both create calls: stride 0 = Conv2d, weight [c_out, c_in, k, k]; 1 | 2 = ConvTranspose2d, weight [c_in, c_out, k, k]
static int conv_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_in, int k, int stride, int act, float slope,
                       int shuffle, int flags, fgmm_conv **out) {
  if (!out) return fail(FGMM_ERR_INVALID, "out == NULL");
  *out = nullptr;
  if (!ctx || !weight) return fail(FGMM_ERR_INVALID, "convolution: null context or weights");
  if (conv_layer_bad(c_out, c_in, k, act, slope, shuffle)) return FGMM_ERR_INVALID;
  if (flags & ~FGMM_CONV_BF16X6) return fail(FGMM_ERR_INVALID, "convolution: unknown flags 0x%x", (unsigned)flags);
  const bool b16 = (flags & FGMM_CONV_BF16X6) != 0;
  if (b16 && conv16_tiles(c_in) > 65535) // (the split kernel's grid: a channel tile per block row)
    return fail(FGMM_ERR_INVALID, "convolution: bf16x6 takes at most %d input channels", 65535 * kHead16BK);
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) % sizeof(float)) return fail(FGMM_ERR_INVALID, "convolution: misaligned tensor");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  fgmm_conv *c = new (std::nothrow) fgmm_conv;
  if (!c) return fail(FGMM_ERR_NOMEM, "convolution");
  c->device = ctx->device, c->c_out = c_out, c->c_in = c_in, c->k = k, c->act = act, c->slope = slope, c->shuffle = shuffle, c->stride = stride;
  const size_t floats = conv_packed_floats(c_out, c_in, k), bias_floats = (size_t)conv_row_tiles(c_out) * 32;
  void *p = nullptr;
  if (dev::malloc_device(&p, (floats + 4) * sizeof(float)) != 0) { // (+ the word the bf16x6 pack kernel flags a weight outside the domain in)
    delete c;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed weights", floats * sizeof(float));
  }
  c->packed = static_cast<float *>(p);
  if (b16 && dev::malloc_device(&c->packed16, conv16_packed_bytes(c_out, c_in, k)) != 0) {
    (void)dev::free_device(p);
    delete c;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed bf16x6 weights", conv16_packed_bytes(c_out, c_in, k));
  }
  float *bp = c->packed + (floats - bias_floats);
  uint32_t *d_bad = reinterpret_cast<uint32_t *>(c->packed + floats);
  uint32_t bad = 0;
  int e = b16 ? dev::memset_async(d_bad, 0, sizeof bad, (dev::Stream)stream) : 0;
  if (!e)
    e = stride == 2 ? launch_deconv_pack(weight, bias, c_out, c_in, k, c->packed, bp, stream)
                    : launch_conv_pack(weight, bias, c_out, c_in, k, stride == 1, c->packed, bp, stream);
  if (!e && b16) e = launch_conv16_pack(weight, c_out, c_in, k, c->packed16, d_bad, stream);
  if (!e) e = dev::stream_sync((dev::Stream)stream); // (the caller may free or overwrite its weights on return)
  if (!e && b16) e = dev::copy_sync(&bad, d_bad, sizeof bad, dev::kD2H);
  if (e || bad) {
    (void)dev::free_device(p);
    if (c->packed16) (void)dev::free_device(c->packed16);
    delete c;
    if (bad) return fail(FGMM_ERR_INVALID, "convolution: a weight is outside the bf16x6 domain (finite, |w| < 0x1.FFp127)");
    return fail(FGMM_ERR_HIP, "packing the convolution's weights: %s", dev::error_string(e));
  }
  *out = c;
  return FGMM_OK;
}

extern "C" {

int fgmm_conv_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_in, int k, int act, float slope, int shuffle,
                     fgmm_conv **out) {
  return conv_create(ctx, stream, weight, bias, c_out, c_in, k, 0, act, slope, shuffle, 0, out);
}

int fgmm_conv_create_ex(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_in, int k, int act, float slope, int shuffle,
                        int flags, fgmm_conv **out) {
  return conv_create(ctx, stream, weight, bias, c_out, c_in, k, 0, act, slope, shuffle, flags, out);
}

int fgmm_conv_create_transposed(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_in, int c_out, int k, int stride, int act,
                                float slope, fgmm_conv **out) {
  if (out) *out = nullptr;
  if (stride != 1 && stride != 2) return fail(FGMM_ERR_INVALID, "transposed convolution: stride = %d (1 or 2)", stride);
  return conv_create(ctx, stream, weight, bias, c_out, c_in, k, stride, act, slope, 1, 0, out);
}

void fgmm_conv_destroy(fgmm_conv *c) {
  if (!c) return;
  {
    DeviceGuard g(c->device);
    (void)dev::free_device(c->packed);
    if (c->packed16) (void)dev::free_device(c->packed16);
  }
  delete c;
}

// bf16x6: bytes of one item's split copy followed by its domain word (0: the sizes overflow), the whole workspace being n of them
static size_t conv16_item_bytes(const fgmm_conv *c, int n, int64_t hw) {
  const int64_t per_pos = (int64_t)conv16_tiles(c->c_in) * 3 * kHead16BK * (int64_t)sizeof(uint16_t);
  if (n <= 0 || hw <= 0 || per_pos > (INT64_MAX / 4 - 64) / hw / n) return 0;
  return (size_t)(per_pos * hw) + kHead16FlagElems * sizeof(uint16_t);
}

// what apply refuses of n > 0 items of hw > 0 positions (at most 2^29) in `patches` patches: 0, or the message.  Blocks are indexed in 30
// bits (head_launch's limit; at most a block per row tile of 32), elements in 63
static const char *conv_sizes_bad(const fgmm_conv *c, int n, int64_t hw, int64_t patches) {
  if (patches > (1ll << 30) / n / ((c->c_out + 31) / 32)) return "n x patches x ceil(c_out / 32) workgroups exceed a grid of 2^30";
  if (hw > INT64_MAX / 8 / n / c->c_out) return "n * channels * h * w overflows";
  return nullptr;
}

// the checks the applies share, then the launches: one, or - b16, a bf16x6 handle's call - the split, the bf16x6 kernel and the exact
// kernel for the items the split flagged
static int conv_run(fgmm_ctx *ctx, void *stream, const fgmm_conv *c, const float *x, int64_t x_item_stride, float *out, int n, int h, int w, bool b16,
                    void *workspace, size_t workspace_bytes) {
  if (!ctx || !c) return fail(FGMM_ERR_INVALID, "convolution: null context or handle");
  if (n < 0 || h < 0 || w < 0) return fail(FGMM_ERR_INVALID, "convolution: n = %d, h = %d, w = %d (each >= 0)", n, h, w);
  if (!x || !out) return fail(FGMM_ERR_INVALID, "convolution: null tensor");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) % sizeof(float)) return fail(FGMM_ERR_INVALID, "convolution: misaligned tensor");
  if (c->device != ctx->device) return fail(FGMM_ERR_INVALID, "convolution: made for device %d, context on %d", c->device, ctx->device);
  // positions of a plane are indexed in 32 bits (the shuffled output's 4 h w too)
  const int64_t hw = (int64_t)h * w;
  if (hw > (INT32_MAX - 256) / 4) return fail(FGMM_ERR_INVALID, "convolution: h * w = %d x %d positions exceed 2^29", h, w);
  if (x_item_stride < (int64_t)c->c_in * hw)
    return fail(FGMM_ERR_INVALID, "convolution: x_item_stride = %lld below c_in * h * w = %lld", (long long)x_item_stride, (long long)c->c_in * hw);
  if (n == 0 || hw == 0) return FGMM_OK;
  const int64_t ph = (h + kConvPR - 1) / kConvPR, pw = (w + kConvPC - 1) / kConvPC;
  if (const char *why = conv_sizes_bad(c, n, hw, ph * pw)) return fail(FGMM_ERR_INVALID, "convolution: n = %d, h = %d, w = %d: %s", n, h, w, why);
  if (x_item_stride > INT64_MAX / 8 / n) return fail(FGMM_ERR_INVALID, "convolution: n * x_item_stride overflows");
  size_t item_bytes = 0;
  if (b16) {
    item_bytes = conv16_item_bytes(c, n, hw);
    if (!item_bytes) return fail(FGMM_ERR_INVALID, "convolution: n * channels * h * w overflows");
    const size_t need = item_bytes * (size_t)n;
    if (!workspace || workspace_bytes < need)
      return fail(FGMM_ERR_INVALID, "convolution: a workspace of %zu bytes, %zu needed (fgmm_conv_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(FGMM_ERR_INVALID, "convolution: the workspace (%zu bytes needed) is not aligned to 16 bytes", need);
  }
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  ConvArgs a;
  memset(&a, 0, sizeof a);
  a.x = x, a.out = out, a.x_item_stride = x_item_stride;
  a.wp = c->packed, a.bp = c->packed + (conv_packed_floats(c->c_out, c->c_in, c->k) - (size_t)conv_row_tiles(c->c_out) * 32);
  a.c_in = c->c_in, a.c_out = c->c_out, a.h = h, a.w = w, a.n_ch = conv_chunks(c->c_in), a.ph = (int32_t)ph, a.pw = (int32_t)pw;
  a.act = c->act, a.shuffle = c->shuffle, a.slope = c->slope;
  if (c->stride == 2) { // out [n, c_out, 2 h, 2 w]: its plane's 4 h w positions are within the limit above
    LAUNCH_TRY(launch_deconv(a, c->k, n, stream));
    return FGMM_OK;
  }
  if (b16) {
    const int64_t xs_stride = (int64_t)(item_bytes / sizeof(uint16_t));
    uint16_t *xs = static_cast<uint16_t *>(workspace);
    for (int i0 = 0; i0 < n; i0 += 65535) // (a grid's third dimension)
      LAUNCH_TRY(launch_head16_split(x + (int64_t)i0 * x_item_stride, xs + i0 * xs_stride, hw, c->c_in, std::min(n - i0, 65535), x_item_stride, xs_stride, stream));
    Conv16Args b;
    memset(&b, 0, sizeof b);
    b.xs = xs, b.xs_stride = xs_stride, b.out = out, b.wp16 = c->packed16, b.bp = a.bp;
    b.c_in = c->c_in, b.c_out = c->c_out, b.h = h, b.w = w, b.n_ct = conv16_tiles(c->c_in), b.ph = a.ph, b.pw = a.pw;
    b.act = c->act, b.shuffle = c->shuffle, b.slope = c->slope;
    LAUNCH_TRY(launch_conv16(b, c->k, n, stream));
    a.only = head16_oob_word(xs, c->c_in, hw), a.only_stride = xs_stride / 2; // (in 32-bit words)
  }
  LAUNCH_TRY(launch_conv(a, c->k, n, stream));
  return FGMM_OK;
}

int fgmm_conv_apply(fgmm_ctx *ctx, void *stream, const fgmm_conv *c, const float *x, int64_t x_item_stride, float *out, int n, int h, int w) {
  if (c && c->packed16) return fail(FGMM_ERR_INVALID, "convolution: a bf16x6 handle needs a workspace: call fgmm_conv_apply_ws");
  return conv_run(ctx, stream, c, x, x_item_stride, out, n, h, w, false, nullptr, 0);
}

size_t fgmm_conv_workspace_bytes(const fgmm_conv *c, int n, int64_t hw) {
  if (!c || !c->packed16 || n <= 0 || hw <= 0 || hw > (INT32_MAX - 256) / 4) return 0;
  // (the grid of an h x w image depends on its two sides: hw positions lie in ceil(hw / 128) patches at the least)
  if (conv_sizes_bad(c, n, hw, (hw + kConvPR * kConvPC - 1) / (kConvPR * kConvPC))) return 0;
  return conv16_item_bytes(c, n, hw) * (size_t)n;
}

int fgmm_conv_apply_ws(fgmm_ctx *ctx, void *stream, const fgmm_conv *c, const float *x, int64_t x_item_stride, float *out, int n, int h, int w,
                       void *workspace, size_t workspace_bytes) {
  return conv_run(ctx, stream, c, x, x_item_stride, out, n, h, w, c && c->packed16, workspace, workspace_bytes);
}

// ---- section 5f: the layer on caller-owned packed weights, and its gradients.  Stream-ordered: validation, the launches, no lock, no wait

size_t fgmm_conv_packed_floats(int c_out, int c_in, int k) {
  if ((k != 3 && k != 5) || c_out < 1 || c_in < 1 || c_out > (1 << 20) || c_in > (1 << 20)) return 0;
  return conv_packed_floats(c_out, c_in, k);
}

int fgmm_conv_pack(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_in, int k, int transposed, float *packed) {
  if (!ctx || !weight || !packed) return fail(FGMM_ERR_INVALID, "convolution: null context, weights or packing");
  if (conv_layer_bad(c_out, c_in, k, FGMM_ACT_NONE, 0.0f, 1)) return FGMM_ERR_INVALID;
  if (transposed != 0 && transposed != 1) return fail(FGMM_ERR_INVALID, "convolution: transposed = %d (0 or 1)", transposed);
  if (transposed && bias) return fail(FGMM_ERR_INVALID, "convolution: the transposed packing takes no bias");
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) % sizeof(float) || reinterpret_cast<uintptr_t>(packed) % 16)
    return fail(FGMM_ERR_INVALID, "convolution: misaligned tensor (the packed weights: 16 bytes)");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  // transposed: the layer from c_out to c_in channels that the data gradient is; `weight` is its [c_in', c_out', k, k] as it stands
  const int po = transposed ? c_in : c_out, pi = transposed ? c_out : c_in;
  float *bp = packed + (conv_packed_floats(po, pi, k) - (size_t)conv_row_tiles(po) * 32);
  LAUNCH_TRY(launch_conv_pack(weight, bias, po, pi, k, transposed != 0, packed, bp, stream));
  return FGMM_OK;
}

int fgmm_conv_apply_packed(fgmm_ctx *ctx, void *stream, const float *packed, int c_out, int c_in, int k, int act, float slope, int shuffle, const float *x,
                           int64_t x_item_stride, float *out, int n, int h, int w) {
  if (!ctx || !packed) return fail(FGMM_ERR_INVALID, "convolution: null context or packed weights");
  if (conv_layer_bad(c_out, c_in, k, act, slope, shuffle)) return FGMM_ERR_INVALID;
  if (reinterpret_cast<uintptr_t>(packed) % 16) return fail(FGMM_ERR_INVALID, "convolution: the packed weights are not aligned to 16 bytes");
  fgmm_conv c; // a handle's view of the caller's packing, for this call
  c.device = ctx->device, c.c_out = c_out, c.c_in = c_in, c.k = k, c.act = act, c.shuffle = shuffle, c.slope = slope;
  c.packed = const_cast<float *>(packed);
  return conv_run(ctx, stream, &c, x, x_item_stride, out, n, h, w, false, nullptr, 0);
}

// what the two gradient calls share after the layer's own refusals: -> 1 to go on, 0 nothing to do, -1 refused (the message set)
static int conv_grad_sizes(const char *what, int c_out, int c_in, int act, float slope, int n, int h, int w) {
  if (act == FGMM_ACT_LEAKY && slope < 0) {
    fail(FGMM_ERR_INVALID, "%s: a negative slope with FGMM_ACT_LEAKY (the saved output's sign is then not the pre-activation's)", what);
    return -1;
  }
  if (n < 0 || h < 0 || w < 0) {
    fail(FGMM_ERR_INVALID, "%s: n = %d, h = %d, w = %d (each >= 0)", what, n, h, w);
    return -1;
  }
  const int64_t hw = (int64_t)h * w;
  if (hw > (INT32_MAX - 256) / 4) {
    fail(FGMM_ERR_INVALID, "%s: h * w = %d x %d positions exceed 2^29", what, h, w);
    return -1;
  }
  if (n == 0 || hw == 0) return 0;
  if (hw > INT64_MAX / 8 / n / std::max(c_out, c_in)) {
    fail(FGMM_ERR_INVALID, "%s: n * channels * h * w overflows", what);
    return -1;
  }
  return 1;
}

int fgmm_conv_dgrad(fgmm_ctx *ctx, void *stream, const float *packed_t, int c_out, int c_in, int k, int act, float slope, int shuffle, const float *gy,
                    const float *out, float *dx, int n, int h, int w) {
  static const char *const what = "convolution data gradient";
  if (!ctx) return fail(FGMM_ERR_INVALID, "%s: null context", what);
  if (conv_layer_bad(c_out, c_in, k, act, slope, shuffle)) return FGMM_ERR_INVALID;
  const int go = conv_grad_sizes(what, c_out, c_in, act, slope, n, h, w);
  if (go < 0) return FGMM_ERR_INVALID;
  if (!packed_t || !gy || !dx || (!out && act != FGMM_ACT_NONE)) return fail(FGMM_ERR_INVALID, "%s: null tensor", what);
  if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dx)) % sizeof(float) ||
      reinterpret_cast<uintptr_t>(packed_t) % 16)
    return fail(FGMM_ERR_INVALID, "%s: misaligned tensor (the packed weights: 16 bytes)", what);
  if (go == 0) return FGMM_OK;
  const int64_t hw = (int64_t)h * w, ph = (h + kConvPR - 1) / kConvPR, pw = (w + kConvPC - 1) / kConvPC;
  if (ph * pw > (1ll << 30) / n / ((c_in + 31) / 32)) return fail(FGMM_ERR_INVALID, "%s: n x patches x ceil(c_in / 32) workgroups exceed a grid of 2^30", what);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  ConvArgs a; // the layer from c_out to c_in channels, on gz
  memset(&a, 0, sizeof a);
  a.x = gy, a.g_out = out, a.out = dx, a.x_item_stride = (int64_t)c_out * hw;
  a.wp = packed_t, a.bp = packed_t + (conv_packed_floats(c_in, c_out, k) - (size_t)conv_row_tiles(c_in) * 32);
  a.c_in = c_out, a.c_out = c_in, a.h = h, a.w = w, a.n_ch = conv_chunks(c_out), a.ph = (int32_t)ph, a.pw = (int32_t)pw;
  a.act = FGMM_ACT_NONE, a.shuffle = 1, a.slope = 0.0f;
  a.g_act = act, a.g_shuffle = shuffle, a.g_slope = slope;
  LAUNCH_TRY(launch_conv_dgrad(a, k, n, stream));
  return FGMM_OK;
}

size_t fgmm_conv_wgrad_workspace(int c_out, int c_in, int k, int n, int h, int w) {
  if ((k != 3 && k != 5) || c_out < 1 || c_in < 1 || c_out > (1 << 20) || c_in > (1 << 20) || n <= 0 || h <= 0 || w <= 0) return 0;
  if ((int64_t)h * w > (INT32_MAX - 256) / 4) return 0;
  const uint64_t floats = (uint64_t)conv_wgrad_slices(n, h, w).S * (uint64_t)c_out * (uint64_t)conv_wgrad_cols(c_in, k);
  return floats > (1ull << 40) ? 0 : (size_t)floats * sizeof(float);
}

int fgmm_conv_wgrad(fgmm_ctx *ctx, void *stream, const float *x, int64_t x_item_stride, const float *gy, const float *out, int c_out, int c_in, int k, int act,
                    float slope, int shuffle, int n, int h, int w, void *workspace, float *dw, float *dbias) {
  static const char *const what = "convolution weight gradient";
  if (!ctx) return fail(FGMM_ERR_INVALID, "%s: null context", what);
  if (conv_layer_bad(c_out, c_in, k, act, slope, shuffle)) return FGMM_ERR_INVALID;
  const int go = conv_grad_sizes(what, c_out, c_in, act, slope, n, h, w);
  if (go < 0) return FGMM_ERR_INVALID;
  if (!x || !gy || !dw || (!out && act != FGMM_ACT_NONE)) return fail(FGMM_ERR_INVALID, "%s: null tensor", what);
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dw) |
       reinterpret_cast<uintptr_t>(dbias)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "%s: misaligned tensor", what);
  if (x_item_stride < (int64_t)c_in * h * w)
    return fail(FGMM_ERR_INVALID, "%s: x_item_stride = %lld below c_in * h * w = %lld", what, (long long)x_item_stride, (long long)c_in * h * w);
  if (go == 0) return FGMM_OK;
  if (x_item_stride > INT64_MAX / 8 / n) return fail(FGMM_ERR_INVALID, "%s: n * x_item_stride overflows", what);
  const size_t need = fgmm_conv_wgrad_workspace(c_out, c_in, k, n, h, w);
  if (!need) return fail(FGMM_ERR_INVALID, "%s: the partial sums of these sizes exceed 2^42 bytes", what);
  if (!workspace) return fail(FGMM_ERR_INVALID, "%s: no workspace, %zu bytes needed (fgmm_conv_wgrad_workspace)", what, need);
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(FGMM_ERR_INVALID, "%s: the workspace is not aligned to 16 bytes", what);
  const ConvWgradSlices sl = conv_wgrad_slices(n, h, w);
  const int64_t bh = (h + kConvPR - 1) / kConvPR, n_cg = (c_in + conv_wgrad_cb(k) - 1) / conv_wgrad_cb(k);
  if (n * bh > INT32_MAX / 2 || sl.S * n_cg * ((c_out + 31) / 32) > (1ll << 30))
    return fail(FGMM_ERR_INVALID, "%s: n * ceil(h / 8) bands beyond 2^30, or slices x column groups x ceil(c_out / 32) workgroups beyond a grid", what);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  ConvWgradArgs a;
  memset(&a, 0, sizeof a);
  a.x = x, a.gy = gy, a.out = out, a.partial = static_cast<float *>(workspace), a.x_item_stride = x_item_stride;
  a.c_in = c_in, a.c_out = c_out, a.h = h, a.w = w, a.bh = (int32_t)bh, a.pw = (w + kConvPC - 1) / kConvPC;
  a.nb = (int32_t)(n * bh), a.B = (int32_t)sl.B, a.S = (int32_t)sl.S;
  a.act = act, a.shuffle = shuffle, a.slope = slope;
  LAUNCH_TRY(launch_conv_wgrad(a, k, stream));
  LAUNCH_TRY(launch_conv_wgrad_finish(a.partial, c_out, c_in, k, a.S, dw, dbias, stream));
  return FGMM_OK;
}

} // extern "C"
