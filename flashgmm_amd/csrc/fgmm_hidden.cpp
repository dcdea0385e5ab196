// fgmm_hidden.cpp — the entry points of the parameter network's hidden layers (include/flashgmm_amd.h section 2c) over fgmm_hidden.hip:
// a handle that owns one layer's packed weights (immutable once made, like a parameter head's) and knows its device's compute units,
// and a STREAM-ORDERED apply - validation, one launch, no workspace, no lock, no wait (a FGMM_HIDDEN_BF16X6 handle, over
// fgmm_hidden16.hip: both packings, and an apply with the caller's workspace - a split per present source, the bf16x6 kernel, the exact
// kernel for the items outside the domain).  A file of its own: the host sources that build against the fake device reference no
// launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

struct fgmm_hidden {
  int device = 0, cus = 0;
  int c_out = 0, c_a = 0, c_b = 0, act = 0;
  float slope = 0.0f;
  float *packed = nullptr; // [wp | bp]
  void *packed16 = nullptr; // FGMM_HIDDEN_BF16X6: the three bf16 parts of the weights (fgmm_hidden16.hip) - the handle holds both packings
};

extern "C" {

int fgmm_hidden_create(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_a, int c_b, int act, float slope,
                       fgmm_hidden **out) {
  return fgmm_hidden_create_ex(ctx, stream, weight, bias, c_out, c_a, c_b, act, slope, 0, out);
}

int fgmm_hidden_create_ex(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_a, int c_b, int act, float slope,
                          int flags, fgmm_hidden **out) {
  if (!out) return fail(FGMM_ERR_INVALID, "out == NULL");
  *out = nullptr;
  if (!ctx || !weight) return fail(FGMM_ERR_INVALID, "hidden layer: null context or weights");
  if (c_out < 1 || c_b < 1 || c_a < 0 || c_out > (1 << 20) || c_a > (1 << 20) || c_b > (1 << 20))
    return fail(FGMM_ERR_INVALID, "hidden layer: c_out = %d, c_a = %d, c_b = %d (c_out >= 1, c_a >= 0, c_b >= 1, each at most 2^20)", c_out, c_a, c_b);
  if (act != FGMM_ACT_NONE && act != FGMM_ACT_LEAKY && act != FGMM_ACT_RELU) return fail(FGMM_ERR_INVALID, "hidden layer: unknown activation %d", act);
  if (!std::isfinite(slope)) return fail(FGMM_ERR_INVALID, "hidden layer: the slope is not finite");
  if (flags & ~FGMM_HIDDEN_BF16X6) return fail(FGMM_ERR_INVALID, "hidden layer: unknown flags 0x%x", (unsigned)flags);
  const bool b16 = (flags & FGMM_HIDDEN_BF16X6) != 0;
  if (b16 && std::max(hidden16_kt(c_a), hidden16_kt(c_b)) > 65535) // (the split kernel's grid: a K tile per block row)
    return fail(FGMM_ERR_INVALID, "hidden layer: bf16x6 takes at most %d channels per source", 65535 * kHead16BK);
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
  if (dev::malloc_device(&p, (floats + 4) * sizeof(float)) != 0) { // (+ the word the bf16x6 pack kernel flags a weight outside the domain in)
    delete h;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed weights", floats * sizeof(float));
  }
  h->packed = static_cast<float *>(p);
  if (b16 && dev::malloc_device(&h->packed16, hidden16_packed_bytes(c_out, c_a, c_b)) != 0) {
    (void)dev::free_device(p);
    delete h;
    return fail(FGMM_ERR_NOMEM, "%zu bytes of device memory for the packed bf16x6 weights", hidden16_packed_bytes(c_out, c_a, c_b));
  }
  uint32_t *d_bad = reinterpret_cast<uint32_t *>(h->packed + floats);
  uint32_t bad = 0;
  e = b16 ? dev::memset_async(d_bad, 0, sizeof bad, (dev::Stream)stream) : 0;
  if (!e) e = launch_hidden_pack(weight, bias, c_out, c_a, c_b, h->packed, h->packed + (floats - bias_floats), stream);
  if (!e && b16) e = launch_hidden16_pack(weight, c_out, c_a, c_b, h->packed16, d_bad, stream);
  if (!e) e = dev::stream_sync((dev::Stream)stream); // (the caller may free or overwrite its weights on return)
  if (!e && b16) e = dev::copy_sync(&bad, d_bad, sizeof bad, dev::kD2H);
  if (e || bad) {
    (void)dev::free_device(p);
    if (h->packed16) (void)dev::free_device(h->packed16);
    delete h;
    if (bad) return fail(FGMM_ERR_INVALID, "hidden layer: a weight is outside the bf16x6 domain (finite, |w| < 0x1.FFp127)");
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
    if (h->packed16) (void)dev::free_device(h->packed16);
  }
  delete h;
}

// bf16x6: bytes of one item's split copies - source a's when present, then source b's, each followed by its domain word (0: the sizes
// overflow), the whole workspace being n of them
static size_t hidden16_item_bytes(const fgmm_hidden *h, bool has_xa, int n, int64_t hw) {
  const int64_t per_pos = (int64_t)((has_xa ? hidden16_kt(h->c_a) : 0) + hidden16_kt(h->c_b)) * 3 * kHead16BK * (int64_t)sizeof(uint16_t);
  if (n <= 0 || hw <= 0 || per_pos > (INT64_MAX / 4 - 64) / hw / n) return 0;
  return (size_t)(per_pos * hw) + (has_xa ? 2 : 1) * kHead16FlagElems * sizeof(uint16_t);
}

// what apply refuses of its sizes (after null and sign checks): 0, or the message's argument
static const char *hidden_sizes_bad(const fgmm_hidden *h, int n, int64_t hw) {
  // blocks are indexed in 30 bits (head_launch's limit; at most a block per row tile of 32), elements in 63
  if (hw > INT64_MAX / 8 / n / std::max(h->c_out, std::max(h->c_a, h->c_b))) return "n * channels * hw overflows";
  if ((hw + 127) / 128 > (1ll << 30) / n / ((h->c_out + 31) / 32)) return "n x ceil(hw / 128) x ceil(c_out / 32) workgroups exceed a grid of 2^30";
  return nullptr;
}

// the checks the applies share, then the launches: one, or - b16, a bf16x6 handle's call - the splits, the bf16x6 kernel and the exact
// kernel for the items the splits flagged
static int hidden_run(fgmm_ctx *ctx, void *stream, const fgmm_hidden *h, const float *xa, const float *xb, float *out, int n, int64_t hw, bool b16,
                      void *workspace, size_t workspace_bytes) {
  if (!ctx || !h) return fail(FGMM_ERR_INVALID, "hidden layer: null context or handle");
  if (n < 0 || hw < 0) return fail(FGMM_ERR_INVALID, "hidden layer: n = %d, hw = %lld (both >= 0)", n, (long long)hw);
  if (xa && h->c_a == 0) return fail(FGMM_ERR_INVALID, "hidden layer: a first source for a layer made with c_a == 0");
  if (!xb || !out) return fail(FGMM_ERR_INVALID, "hidden layer: null tensor");
  if ((reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(out)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "hidden layer: misaligned tensor");
  if (h->device != ctx->device) return fail(FGMM_ERR_INVALID, "hidden layer: made for device %d, context on %d", h->device, ctx->device);
  if (n == 0 || hw == 0) return FGMM_OK;
  if (const char *why = hidden_sizes_bad(h, n, hw)) return fail(FGMM_ERR_INVALID, "hidden layer: n = %d, hw = %lld: %s", n, (long long)hw, why);
  const int64_t pt = (hw + 127) / 128;
  size_t item_bytes = 0;
  if (b16) {
    item_bytes = hidden16_item_bytes(h, xa != nullptr, n, hw);
    if (!item_bytes) return fail(FGMM_ERR_INVALID, "hidden layer: n * channels * hw overflows");
    const size_t need = item_bytes * (size_t)n;
    if (!workspace || workspace_bytes < need)
      return fail(FGMM_ERR_INVALID, "hidden layer: a workspace of %zu bytes, %zu needed (fgmm_hidden_workspace_bytes)", workspace ? workspace_bytes : (size_t)0, need);
    if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(FGMM_ERR_INVALID, "hidden layer: the workspace (%zu bytes needed) is not aligned to 16 bytes", need);
  }
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
  if (b16) {
    // item i of the workspace: [source a's split copy | its domain word | source b's | its domain word], the first two only with xa
    const int64_t xs_stride = (int64_t)(item_bytes / sizeof(uint16_t));
    uint16_t *xsa = static_cast<uint16_t *>(workspace), *xsb = xsa + (xa ? head16_split_elems(h->c_a, hw) + kHead16FlagElems : 0);
    for (int i0 = 0; i0 < n; i0 += 65535) { // (a grid's third dimension)
      const int cnt = std::min(n - i0, 65535);
      if (xa) LAUNCH_TRY(launch_head16_split(xa + (int64_t)i0 * h->c_a * hw, xsa + i0 * xs_stride, hw, h->c_a, cnt, (int64_t)h->c_a * hw, xs_stride, stream));
      LAUNCH_TRY(launch_head16_split(xb + (int64_t)i0 * h->c_b * hw, xsb + i0 * xs_stride, hw, h->c_b, cnt, (int64_t)h->c_b * hw, xs_stride, stream));
    }
    Hidden16Args b;
    memset(&b, 0, sizeof b);
    b.xsa = xsa, b.xsb = xsb, b.xs_stride = xs_stride, b.out = out, b.wp16 = h->packed16, b.bp = a.bp, b.hw = hw;
    b.c_a = h->c_a, b.c_b = h->c_b, b.c_out = h->c_out;
    b.kta = xa ? hidden16_kt(h->c_a) : 0, b.n_kt = b.kta + hidden16_kt(h->c_b);
    b.kt_all = hidden16_kt(h->c_a) + hidden16_kt(h->c_b), b.kt0 = b.kt_all - b.n_kt; // an absent source's tiles are skipped
    b.pt = a.pt, b.act = h->act, b.slope = h->slope;
    LAUNCH_TRY(launch_hidden16(b, n, h->cus, stream));
    a.only_b = head16_oob_word(xsb, h->c_b, hw), a.only = xa ? head16_oob_word(xsa, h->c_a, hw) : a.only_b;
    a.only_stride = xs_stride / 2; // (in 32-bit words)
  }
  const bool vec = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb)) % 16 == 0;
  LAUNCH_TRY(launch_hidden(a, n, h->cus, vec, stream));
  return FGMM_OK;
}

int fgmm_hidden_apply(fgmm_ctx *ctx, void *stream, const fgmm_hidden *h, const float *xa, const float *xb, float *out, int n, int64_t hw) {
  if (h && h->packed16) return fail(FGMM_ERR_INVALID, "hidden layer: a bf16x6 handle needs a workspace: call fgmm_hidden_apply_ws");
  return hidden_run(ctx, stream, h, xa, xb, out, n, hw, false, nullptr, 0);
}

size_t fgmm_hidden_workspace_bytes(const fgmm_hidden *h, int has_xa, int n, int64_t hw) {
  if (!h || !h->packed16 || n <= 0 || hw <= 0 || (has_xa && h->c_a == 0) || hidden_sizes_bad(h, n, hw)) return 0;
  return hidden16_item_bytes(h, has_xa != 0, n, hw) * (size_t)n;
}

int fgmm_hidden_apply_ws(fgmm_ctx *ctx, void *stream, const fgmm_hidden *h, const float *xa, const float *xb, float *out, int n, int64_t hw,
                         void *workspace, size_t workspace_bytes) {
  return hidden_run(ctx, stream, h, xa, xb, out, n, hw, h && h->packed16, workspace, workspace_bytes);
}

// ---- section 2d: caller-owned packed weights (the gradients themselves: fgmm_hidden_grad.cpp) ---------------------------------------
static bool hidden_sizes_ok(int c_out, int c_a, int c_b) { return c_out >= 1 && c_b >= 1 && c_a >= 0 && c_out <= (1 << 20) && c_a <= (1 << 20) && c_b <= (1 << 20); }

size_t fgmm_hidden_packed_floats(int c_out, int c_a, int c_b) { return hidden_sizes_ok(c_out, c_a, c_b) ? hidden_packed_floats(c_out, c_a, c_b) : 0; }

int fgmm_hidden_pack(fgmm_ctx *ctx, void *stream, const float *weight, const float *bias, int c_out, int c_a, int c_b, int transposed, float *packed) {
  if (!ctx || !weight || !packed || !hidden_sizes_ok(c_out, c_a, c_b) || (transposed & ~1) || (transposed && bias))
    return fail(FGMM_ERR_INVALID, "hidden layer: bad argument to pack (null tensor, sizes, a bias with the transposed form)");
  if ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias) | reinterpret_cast<uintptr_t>(packed)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "hidden layer: misaligned tensor");
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  if (transposed) LAUNCH_TRY(launch_hidden_pack_t(weight, c_out, c_a, c_b, packed, stream));
  else LAUNCH_TRY(launch_hidden_pack(weight, bias, c_out, c_a, c_b, packed, packed + (hidden_packed_floats(c_out, c_a, c_b) - (size_t)hidden_row_tiles(c_out) * 32), stream));
  return FGMM_OK;
}

int fgmm_hidden_apply_packed(fgmm_ctx *ctx, void *stream, const float *packed, int c_out, int c_a, int c_b, int act, float slope, const float *xa,
                             const float *xb, float *out, int n, int64_t hw) {
  if (!ctx || !hidden_sizes_ok(c_out, c_a, c_b)) return fail(FGMM_ERR_INVALID, "hidden layer: bad argument (context, channel counts)");
  if (act != FGMM_ACT_NONE && act != FGMM_ACT_LEAKY && act != FGMM_ACT_RELU) return fail(FGMM_ERR_INVALID, "hidden layer: unknown activation %d", act);
  if (!std::isfinite(slope)) return fail(FGMM_ERR_INVALID, "hidden layer: the slope is not finite");
  if (!packed || reinterpret_cast<uintptr_t>(packed) % 16) return fail(FGMM_ERR_INVALID, "hidden layer: null packed weights, or not aligned to 16 bytes");
  fgmm_hidden h; // the handle's view of the caller's buffer: nothing here is owned
  h.device = ctx->device, h.c_out = c_out, h.c_a = c_a, h.c_b = c_b, h.act = act, h.slope = slope;
  h.packed = const_cast<float *>(packed);
  const int e = hidden_device_cus(ctx->device, &h.cus);
  if (e || h.cus < 1) return fail(FGMM_ERR_HIP, "hidden layer: the device's compute units: %s", dev::error_string(e));
  return hidden_run(ctx, stream, &h, xa, xb, out, n, hw, false, nullptr, 0);
}

} // extern "C"
