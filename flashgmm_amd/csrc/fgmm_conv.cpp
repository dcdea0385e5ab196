// fgmm_conv.cpp — the entry points of the dense 3x3 / 5x5 convolution layers (include/flashgmm_amd.h section 5d) over fgmm_conv.hip: a
// handle that owns one layer's packed weights (immutable once made, like a hidden layer's) and a STREAM-ORDERED apply - validation, one
// launch, no workspace, no lock, no wait.  A file of its own: the host sources that build against the fake device reference no launcher
// of these.  The transposed layers of section 5e (fgmm_conv_create_transposed) are the same handle: stride 1 on fgmm_conv.hip's kernel
// over the flipped pack, stride 2 on fgmm_deconv.hip; apply dispatches on the handle.
#include "fgmm_ctx.h"

using namespace fgmm;

struct fgmm_conv {
  int device = 0;
  int c_out = 0, c_in = 0, k = 0, act = 0, shuffle = 1;
  int stride = 0; // 0: a Conv2d layer (section 5d); 1 | 2: a ConvTranspose2d layer of that stride (section 5e)
  float slope = 0.0f;
  float *packed = nullptr; // [wp | bp]
};

// both create calls: stride 0 = Conv2d, weight [c_out, c_in, k, k]; 1 | 2 = ConvTranspose2d, weight [c_in, c_out, k, k]
static int conv_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_in, int k, int stride, int act, float slope,
                       int shuffle, fgmm_conv **out) {
  if (!out) return fail(FGMM_ERR_INVALID, "out == NULL");
  *out = nullptr;
  if (!ctx || !weight) return fail(FGMM_ERR_INVALID, "convolution: null context or weights");
  if (k != 3 && k != 5) return fail(FGMM_ERR_INVALID, "convolution: k = %d (3 or 5)", k);
  if (c_out < 1 || c_in < 1 || c_out > (1 << 20) || c_in > (1 << 20))
    return fail(FGMM_ERR_INVALID, "convolution: c_out = %d, c_in = %d (each from 1 to 2^20)", c_out, c_in);
  if (act != FGMM_ACT_NONE && act != FGMM_ACT_LEAKY && act != FGMM_ACT_RELU) return fail(FGMM_ERR_INVALID, "convolution: unknown activation %d", act);
  if (!std::isfinite(slope)) return fail(FGMM_ERR_INVALID, "convolution: the slope is not finite");
  if (shuffle != 1 && shuffle != 2) return fail(FGMM_ERR_INVALID, "convolution: shuffle = %d (1 or 2)", shuffle);
  if (shuffle == 2 && c_out % 4) return fail(FGMM_ERR_INVALID, "convolution: shuffle 2 needs c_out = %d to be a multiple of 4", c_out);
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) % sizeof(float)) return fail(FGMM_ERR_INVALID, "convolution: misaligned tensor");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  fgmm_conv *c = new (std::nothrow) fgmm_conv;
  if (!c) return fail(FGMM_ERR_NOMEM, "convolution");
  c->device = ctx->device, c->c_out = c_out, c->c_in = c_in, c->k = k, c->act = act, c->slope = slope, c->shuffle = shuffle, c->stride = stride;
  const size_t floats = conv_packed_floats(c_out, c_in, k), bias_floats = (size_t)conv_row_tiles(c_out) * 32;
  void *p = nullptr;
  if (dev::malloc_device(&p, floats * sizeof(float)) != 0) {
    delete c;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed weights", floats * sizeof(float));
  }
  c->packed = static_cast<float *>(p);
  float *bp = c->packed + (floats - bias_floats);
  int e = stride == 2 ? launch_deconv_pack(weight, bias, c_out, c_in, k, c->packed, bp, stream)
                      : launch_conv_pack(weight, bias, c_out, c_in, k, stride == 1, c->packed, bp, stream);
  if (!e) e = dev::stream_sync((dev::Stream)stream); // (the caller may free or overwrite its weights on return)
  if (e) {
    (void)dev::free_device(p);
    delete c;
    return fail(FGMM_ERR_HIP, "packing the convolution's weights: %s", dev::error_string(e));
  }
  *out = c;
  return FGMM_OK;
}

extern "C" {

int fgmm_conv_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_in, int k, int act, float slope, int shuffle,
                     fgmm_conv **out) {
  return conv_create(ctx, stream, weight, bias, c_out, c_in, k, 0, act, slope, shuffle, out);
}

int fgmm_conv_create_transposed(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_in, int c_out, int k, int stride, int act,
                                float slope, fgmm_conv **out) {
  if (out) *out = nullptr;
  if (stride != 1 && stride != 2) return fail(FGMM_ERR_INVALID, "transposed convolution: stride = %d (1 or 2)", stride);
  return conv_create(ctx, stream, weight, bias, c_out, c_in, k, stride, act, slope, 1, out);
}

void fgmm_conv_destroy(fgmm_conv *c) {
  if (!c) return;
  {
    DeviceGuard g(c->device);
    (void)dev::free_device(c->packed);
  }
  delete c;
}

int fgmm_conv_apply(fgmm_ctx *ctx, void *stream, const fgmm_conv *c, const float *x, int64_t x_item_stride, float *out, int n, int h, int w) {
  if (!ctx || !c) return fail(FGMM_ERR_INVALID, "convolution: null context or handle");
  if (n < 0 || h < 0 || w < 0) return fail(FGMM_ERR_INVALID, "convolution: n = %d, h = %d, w = %d (each >= 0)", n, h, w);
  if (!x || !out) return fail(FGMM_ERR_INVALID, "convolution: null tensor");
  if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) % sizeof(float)) return fail(FGMM_ERR_INVALID, "convolution: misaligned tensor");
  if (c->device != ctx->device) return fail(FGMM_ERR_INVALID, "convolution: made for device %d, context on %d", c->device, ctx->device);
  // positions of a plane are indexed in 32 bits (the shuffled output's 4 h w too), blocks in 30 (head_launch's limit), elements in 63
  const int64_t hw = (int64_t)h * w;
  if (hw > (INT32_MAX - 256) / 4) return fail(FGMM_ERR_INVALID, "convolution: h * w = %d x %d positions exceed 2^29", h, w);
  if (x_item_stride < (int64_t)c->c_in * hw)
    return fail(FGMM_ERR_INVALID, "convolution: x_item_stride = %lld below c_in * h * w = %lld", (long long)x_item_stride, (long long)c->c_in * hw);
  if (n == 0 || hw == 0) return FGMM_OK;
  const int64_t ph = (h + kConvPR - 1) / kConvPR, pw = (w + kConvPC - 1) / kConvPC, n_rt = (c->c_out + 31) / 32; // (at most a block per row tile of 32)
  if (ph * pw > (1ll << 30) / n / n_rt)
    return fail(FGMM_ERR_INVALID, "convolution: %d x %lld x %lld workgroups exceed a grid of 2^30", n, (long long)(ph * pw), (long long)n_rt);
  if (hw > INT64_MAX / 8 / n / c->c_out || x_item_stride > INT64_MAX / 8 / n) return fail(FGMM_ERR_INVALID, "convolution: n * channels * h * w overflows");
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
  LAUNCH_TRY(launch_conv(a, c->k, n, stream));
  return FGMM_OK;
}

} // extern "C"
