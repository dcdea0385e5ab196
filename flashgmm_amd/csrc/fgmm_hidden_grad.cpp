// fgmm_hidden_grad.cpp — the entry points of the hidden layers' gradients (include/flashgmm_amd.h section 2d) over fgmm_hidden_grad.hip:
// STREAM-ORDERED calls on caller-owned memory - validation, the launches, no lock, no wait.  (The packings and the forward over a
// caller-owned packing, fgmm_hidden_pack and fgmm_hidden_apply_packed, sit beside the handle in fgmm_hidden.cpp.)  A file of its own:
// the host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

// what the two gradient calls share (after the context): sizes, activation, the positions.  -> P = n * hw (0: nothing to do), or -1 with
// the error set
static int64_t hidden_grad_positions(const char *what, int c_out, int c_a, int c_b, int act, float slope, int n, int64_t hw) {
  if (c_out < 1 || c_b < 1 || c_a < 0 || c_out > (1 << 20) || c_a > (1 << 20) || c_b > (1 << 20) || n < 0 || hw < 0) {
    fail(FGMM_ERR_INVALID, "%s: c_out = %d, c_a = %d, c_b = %d, n = %d, hw = %lld (c_out >= 1, c_a >= 0, c_b >= 1, each at most 2^20; n, hw >= 0)", what, c_out,
         c_a, c_b, n, (long long)hw);
    return -1;
  }
  if (act != FGMM_ACT_NONE && act != FGMM_ACT_LEAKY && act != FGMM_ACT_RELU) {
    fail(FGMM_ERR_INVALID, "%s: unknown activation %d", what, act);
    return -1;
  }
  if (!std::isfinite(slope) || (act == FGMM_ACT_LEAKY && slope < 0)) {
    fail(FGMM_ERR_INVALID, "%s: the slope is not finite, or negative with FGMM_ACT_LEAKY (the saved output's sign is then not the pre-activation's)", what);
    return -1;
  }
  if (n == 0 || hw == 0) return 0;
  if (hw > (INT32_MAX - 256) / n) {
    fail(FGMM_ERR_INVALID, "%s: n * hw = %d x %lld positions exceed 2^31", what, n, (long long)hw);
    return -1;
  }
  if (hw > INT64_MAX / 8 / n / std::max(c_out, std::max(c_a, c_b))) {
    fail(FGMM_ERR_INVALID, "%s: n * channels * hw overflows", what);
    return -1;
  }
  return (int64_t)n * hw;
}

extern "C" {

int fgmm_hidden_dgrad(fgmm_ctx *ctx, void *stream, const float *packed_t, int c_out, int c_a, int c_b, int act, float slope, const float *gy,
                      const float *out, float *dxa, float *dxb, int n, int64_t hw) {
  static const char *const what = "hidden layer data gradient";
  if (!ctx) return fail(FGMM_ERR_INVALID, "%s: null context", what);
  const int64_t P = hidden_grad_positions(what, c_out, c_a, c_b, act, slope, n, hw);
  if (P < 0) return FGMM_ERR_INVALID;
  if (dxa && c_a == 0) return fail(FGMM_ERR_INVALID, "%s: dxa for a layer with c_a == 0", what);
  if (P == 0) return FGMM_OK;
  if (!dxa && !dxb) return fail(FGMM_ERR_INVALID, "%s: neither dxa nor dxb", what);
  if (!packed_t || !gy || (!out && act != FGMM_ACT_NONE)) return fail(FGMM_ERR_INVALID, "%s: null tensor", what);
  if ((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dxa) | reinterpret_cast<uintptr_t>(dxb)) % sizeof(float) ||
      reinterpret_cast<uintptr_t>(packed_t) % 16)
    return fail(FGMM_ERR_INVALID, "%s: misaligned tensor (the packed weights: 16 bytes)", what);
  const int64_t pt = (hw + 127) / 128;
  if (pt > (1ll << 30) / n / ((c_a + c_b + 31) / 32)) // (at most a block per row tile of 32)
    return fail(FGMM_ERR_INVALID, "%s: n x ceil(hw / 128) x ceil((c_a + c_b) / 32) workgroups exceed a grid of 2^30", what);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  int cus = 0;
  const int e = hidden_device_cus(ctx->device, &cus);
  if (e || cus < 1) return fail(FGMM_ERR_HIP, "%s: the device's compute units: %s", what, dev::error_string(e));
  HiddenDgradArgs a;
  memset(&a, 0, sizeof a);
  a.gy = gy, a.out = out, a.dxa = dxa, a.dxb = dxb, a.wp = packed_t, a.hw = hw;
  a.c_a = c_a, a.c_b = c_b, a.c_out = c_out;
  a.r0 = dxa ? 0 : c_a, a.r1 = dxb ? c_a + c_b : c_a;
  a.n_kt = (c_out + kMfma32BK - 1) / kMfma32BK, a.pt = (int32_t)pt;
  a.act = act, a.slope = slope;
  const bool vec = hw % 4 == 0 && (reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(act != FGMM_ACT_NONE ? out : nullptr)) % 16 == 0;
  LAUNCH_TRY(launch_hidden_dgrad(a, n, cus, vec, stream));
  return FGMM_OK;
}

size_t fgmm_hidden_wgrad_workspace(int c_out, int c_a, int c_b, int has_xa, int n, int64_t hw) {
  const int64_t P = hidden_grad_positions("hidden layer weight gradient", c_out, c_a, c_b, FGMM_ACT_NONE, 0.0f, n, hw);
  if (P <= 0 || (has_xa && c_a == 0)) return 0;
  return (size_t)ckbd_wgrad_slices(P).S * (size_t)c_out * ((size_t)c_a + c_b + 1) * sizeof(float);
}

int fgmm_hidden_wgrad(fgmm_ctx *ctx, void *stream, const float *xa, const float *xb, const float *gy, const float *out, int c_out, int c_a, int c_b, int act,
                      float slope, int n, int64_t hw, float *dweight, float *dbias, void *workspace, size_t workspace_bytes) {
  static const char *const what = "hidden layer weight gradient";
  if (!ctx) return fail(FGMM_ERR_INVALID, "%s: null context", what);
  const int64_t P = hidden_grad_positions(what, c_out, c_a, c_b, act, slope, n, hw);
  if (P < 0) return FGMM_ERR_INVALID;
  if (xa && c_a == 0) return fail(FGMM_ERR_INVALID, "%s: a first source for a layer with c_a == 0", what);
  if (P == 0) return FGMM_OK;
  if (!dweight && !dbias) return fail(FGMM_ERR_INVALID, "%s: neither dweight nor dbias", what);
  if (!gy || (dweight && !xb) || (!out && act != FGMM_ACT_NONE)) return fail(FGMM_ERR_INVALID, "%s: null tensor", what);
  if ((reinterpret_cast<uintptr_t>(xa) | reinterpret_cast<uintptr_t>(xb) | reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(out) |
       reinterpret_cast<uintptr_t>(dweight) | reinterpret_cast<uintptr_t>(dbias)) % sizeof(float))
    return fail(FGMM_ERR_INVALID, "%s: misaligned tensor", what);
  const CkbdWgradSlices sl = ckbd_wgrad_slices(P);
  const size_t need = (size_t)sl.S * (size_t)c_out * ((size_t)c_a + c_b + 1) * sizeof(float);
  if (!workspace || workspace_bytes < need) return fail(FGMM_ERR_INVALID, "%s: a workspace of %zu bytes, %zu needed", what, workspace ? workspace_bytes : (size_t)0, need);
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return fail(FGMM_ERR_INVALID, "%s: the workspace is not aligned to 16 bytes", what);
  const int mta = (c_a + 31) / 32, mtb = (c_b + 31) / 32;
  const int64_t col_groups = ((int64_t)mta + mtb + 4) / 4, n_rt = (c_out + 31) / 32; // (at most a block per row tile)
  if (sl.S * col_groups * n_rt > (1ll << 30))
    return fail(FGMM_ERR_INVALID, "%s: %lld x %lld x %lld workgroups exceed a grid", what, (long long)sl.S, (long long)col_groups, (long long)n_rt);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select HIP device %d", ctx->device);
  HiddenWgradArgs a;
  memset(&a, 0, sizeof a);
  a.xa = dweight ? xa : nullptr, a.xb = xb, a.gy = gy, a.out = out, a.partial = static_cast<float *>(workspace);
  a.c_a = c_a, a.c_b = c_b, a.c_out = c_out, a.hw = (int32_t)hw, a.mta = mta, a.mtb = mtb;
  // the column tiles: source a's (skipped when it is absent), source b's, the bias' last
  a.col0 = !dweight ? mta + mtb : (xa ? 0 : mta);
  a.n_col = (mta + mtb - std::min(a.col0, mta + mtb)) + (dbias ? 1 : 0);
  a.P = (int32_t)P, a.L = (int32_t)sl.L, a.S = (int32_t)sl.S;
  a.act = act, a.slope = slope;
  LAUNCH_TRY(launch_hidden_wgrad(a, stream));
  LAUNCH_TRY(launch_hidden_wgrad_finish(a.partial, c_a, c_b, c_out, xa != nullptr, a.S, dweight, dbias, stream));
  return FGMM_OK;
}

} // extern "C"
