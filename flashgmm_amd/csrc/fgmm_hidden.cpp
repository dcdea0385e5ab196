// fgmm_hidden.cpp — the entry points of the parameter network's hidden layers (include/flashgmm_amd.h section 2c) over fgmm_hidden.hip:
// a handle that owns one layer's packed weights (immutable once made, like a parameter head's) and knows its device's compute units,
// and a STREAM-ORDERED apply - validation, one launch, no workspace, no lock, no wait.  A file of its own: the host sources that
// build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

struct fgmm_hidden {
  int device = 0, cus = 0;
  int c_out = 0, c_a = 0, c_b = 0, act = 0;
  float slope = 0.0f;
  float *packed = nullptr; // [wp | bp]
};

extern "C" {

int fgmm_hidden_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_a, int c_b, int act, float slope,
                       fgmm_hidden **out) {
  if (!out) return fail(FGMM_ERR_INVALID, "out == NULL");
  *out = nullptr;
  if (!ctx || !weight) return fail(FGMM_ERR_INVALID, "hidden layer: null context or weights");
  if (c_out < 1 || c_b < 1 || c_a < 0 || c_out > (1 << 20) || c_a > (1 << 20) || c_b > (1 << 20))
    return fail(FGMM_ERR_INVALID, "hidden layer: c_out = %d, c_a = %d, c_b = %d (c_out >= 1, c_a >= 0, c_b >= 1, each at most 2^20)", c_out, c_a, c_b);
  if (act != FGMM_ACT_NONE && act != FGMM_ACT_LEAKY && act != FGMM_ACT_RELU) return fail(FGMM_ERR_INVALID, "hidden layer: unknown activation %d", act);
  if (!std::isfinite(slope)) return fail(FGMM_ERR_INVALID, "hidden layer: the slope is not finite");
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) % sizeof(float)) return fail(FGMM_ERR_INVALID, "hidden layer: misaligned tensor");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  fgmm_hidden *h = new (std::nothrow) fgmm_hidden;
  if (!h) return fail(FGMM_ERR_NOMEM, "hidden layer");
  h->device = ctx->device, h->c_out = c_out, h->c_a = c_a, h->c_b = c_b, h->act = act, h->slope = slope;
  int e = hidden_device_cus(ctx->device, &h->cus);
  if (e || h->cus < 1) {
    delete h;
    return fail(FGMM_ERR_HIP, "hidden layer: the device's compute units: %s", dev::error_string(e));
  }
  const size_t floats = hidden_packed_floats(c_out, c_a, c_b), bias_floats = (size_t)hidden_row_tiles(c_out) * 32;
  void *p = nullptr;
  if (dev::malloc_device(&p, floats * sizeof(float)) != 0) {
    delete h;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed weights", floats * sizeof(float));
  }
  h->packed = static_cast<float *>(p);
  e = launch_hidden_pack(weight, bias, c_out, c_a, c_b, h->packed, h->packed + (floats - bias_floats), stream);
  if (!e) e = dev::stream_sync((dev::Stream)stream); // (the caller may free or overwrite its weights on return)
  if (e) {
    (void)dev::free_device(p);
    delete h;
    return fail(FGMM_ERR_HIP, "packing the hidden layer's weights: %s", dev::error_string(e));
  }
  *out = h;
  return FGMM_OK;
}

void fgmm_hidden_destroy(fgmm_hidden *h) {
  if (!h) return;
  {
    DeviceGuard g(h->device);
    (void)dev::free_device(h->packed);
  }
  delete h;
}

int fgmm_hidden_apply(fgmm_ctx *ctx, void *stream, const fgmm_hidden *h, const float *xa, const float *xb, float *out, int n, int64_t hw) {
  if (!ctx || !h) return fail(FGMM_ERR_INVALID, "hidden layer: null context or handle");
  if (n < 0 || hw < 0) return fail(FGMM_ERR_INVALID, "hidden layer: n = %d, hw = %lld (both >= 0)", n, (long long)hw);
  if (xa && h->c_a == 0) return fail(FGMM_ERR_INVALID, "hidden layer: a first source for a layer made with c_a == 0");
  if (!xb || !out) return fail(FGMM_ERR_INVALID, "hidden layer: null tensor");
  if ((reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(out)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "hidden layer: misaligned tensor");
  if (h->device != ctx->device) return fail(FGMM_ERR_INVALID, "hidden layer: made for device %d, context on %d", h->device, ctx->device);
  if (n == 0 || hw == 0) return FGMM_OK;
  // blocks are indexed in 30 bits (head_launch's limit; at most a block per row tile of 32), elements in 63
  if (hw > INT64_MAX / 8 / n / std::max(h->c_out, std::max(h->c_a, h->c_b))) return fail(FGMM_ERR_INVALID, "hidden layer: n * channels * hw overflows");
  const int64_t pt = (hw + 127) / 128, n_rt = (h->c_out + 31) / 32;
  if (pt > (1ll << 30) / n / n_rt) return fail(FGMM_ERR_INVALID, "hidden layer: %d x %lld x %lld workgroups exceed a grid", n, (long long)pt, (long long)n_rt);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  const int kta = (h->c_a + kMfma32BK - 1) / kMfma32BK, ktb = (h->c_b + kMfma32BK - 1) / kMfma32BK;
  HiddenArgs a;
  memset(&a, 0, sizeof a);
  a.xa = xa, a.xb = xb, a.out = out;
  a.wp = h->packed + (xa ? 0 : (size_t)kta * 32 * kMfma32BK); // an absent source's tiles are not part of the chain
  a.bp = h->packed + (hidden_packed_floats(h->c_out, h->c_a, h->c_b) - (size_t)hidden_row_tiles(h->c_out) * 32);
  a.hw = hw, a.rt_words = (int64_t)(kta + ktb) * (32 * kMfma32BK / 4);
  a.c_a = h->c_a, a.c_b = h->c_b, a.c_out = h->c_out;
  a.kta = xa ? kta : 0, a.n_kt = a.kta + ktb, a.pt = (int32_t)pt;
  a.act = h->act, a.slope = h->slope;
  const bool vec = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb)) % 16 == 0;
  LAUNCH_TRY(launch_hidden(a, n, h->cus, vec, stream));
  return FGMM_OK;
}

} // extern "C"
