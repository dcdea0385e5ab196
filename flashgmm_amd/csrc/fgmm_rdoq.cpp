// fgmm_rdoq.cpp — rate-distortion optimised quantisation of a batch of latents (include/flashgmm_amd.h section 3c).  The size
// estimate's front half (fgmm_estimate.cpp: quant_stats_kernel and chan_compact_kernel give the channels the compress call would
// code for y), then rdoq_kernel (fgmm_rdoq.hip) in place of rate_kernel, then the census once more, over y_rdo: its abs_max and
// zero_bitmap are what a compress call of y_rdo will return.  Nothing but the per-channel census and sums crosses PCIe.  A file of
// its own, as fgmm_estimate.cpp: the host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

namespace {

struct RdoqOff { // workspace offsets of one item: the census of y, the census of y_rdo, the sums
  CensusOff census, census2;
  size_t o_before, o_after, o_changed;
};

} // namespace

// lambdas[i * lambda_stride] is item i's lambda (stride 0: one for the call, fgmm_gmc_rdoq_batch; 1: the budget call of section 3d, whose
// groups end at lambdas of their own): consecutive items of one lambda share a launch of rdoq_kernel, everything else is once per call
int fgmm::rdoq_run(fgmm_ctx *ctx, dev::Stream stream, fgmm_rdoq_item *items, int count, int mode, int clamp, const double *lambdas, int lambda_stride) {
  int rc;
  if ((rc = ensure_rate_table(ctx))) return rc;
  // ---- workspace: [EncDesc x count (y)][EncDesc x count (y_rdo)][RdoqDesc x count][small: per item the arrays of RdoqOff] ----------
  Arena ar;
  const size_t o_descs = ar.take(sizeof(EncDesc) * (size_t)count);
  const size_t o_descs2 = ar.take(sizeof(EncDesc) * (size_t)count);
  const size_t o_qdescs = ar.take(sizeof(RdoqDesc) * (size_t)count);
  const size_t o_small = ar.take(0);
  std::vector<RdoqOff> off((size_t)count);
  int M_max = 0;
  int64_t hw_max = 0, n_max = 0;
  for (int i = 0; i < count; ++i) {
    const fgmm_rdoq_item &it = items[i];
    RdoqOff &o = off[(size_t)i];
    o.census = census_take(ar, it.M);
    o.census2 = census_take(ar, it.M);
    o.o_before = ar.take(sizeof(unsigned long long) * it.M, 16);
    o.o_after = ar.take(sizeof(unsigned long long) * it.M, 16);
    o.o_changed = ar.take(sizeof(unsigned long long) * it.M, 16);
    M_max = std::max(M_max, it.M);
    hw_max = std::max(hw_max, it.hw);
    n_max = std::max(n_max, (int64_t)it.M * it.hw);
  }
  const size_t small_bytes = ar.off - o_small;
  if ((rc = ctx->ensure_device(ar.off)) || (rc = ctx->ensure_host(ar.off)) || (rc = ctx->ensure_events(1))) return rc;
  // ---- descriptors ------------------------------------------------------------------------------------------------------------
  EncDesc *hd = reinterpret_cast<EncDesc *>(ctx->h_ws + o_descs);
  EncDesc *hd2 = reinterpret_cast<EncDesc *>(ctx->h_ws + o_descs2);
  RdoqDesc *hq = reinterpret_cast<RdoqDesc *>(ctx->h_ws + o_qdescs);
  const bool f16 = items[0].params.dtype == FGMM_F16;
  bool vec4 = true, linear = true;
  for (int i = 0; i < count; ++i) {
    const fgmm_rdoq_item &it = items[i];
    const RdoqOff &o = off[(size_t)i];
    EncDesc &d = hd[i];
    census_desc(d, ctx, o.census, it.y, &it.params, it.M, it.hw, clamp);
    census_desc(hd2[i], ctx, o.census2, it.y_rdo, nullptr, it.M, it.hw, clamp); // the census of y_rdo
    RdoqDesc &q = hq[i];
    q.y_out = it.y_rdo;
    q.chan_before = reinterpret_cast<unsigned long long *>(ctx->d_ws + o.o_before);
    q.chan_after = reinterpret_cast<unsigned long long *>(ctx->d_ws + o.o_after);
    q.chan_changed = reinterpret_cast<unsigned long long *>(ctx->d_ws + o.o_changed);
    vec4 = vec4 && enc_vec4_ok(d, q.y_out, f16);
  }
  const int vec = vec4 ? 4 : 1;
  for (int i = 0; i < count; ++i) linear = linear && items[i].hw % (64 * vec) == 0;
  // ---- kernels, the small region back -----------------------------------------------------------------------------------------
  DEV_TRY(dev::copy_async(ctx->d_ws + o_descs, hd, o_small - o_descs, dev::kH2D, stream)); // (the three descriptor arrays: one copy)
  DEV_TRY(dev::memset_async(ctx->d_ws + o_small, 0, small_bytes, stream));
  for (int i = 0; i < count; ++i) // +0.0 in the channels that are not coded (all of their round(y) are zeros); rdoq_kernel writes the others
    if ((int64_t)items[i].M * items[i].hw)
      DEV_TRY(dev::memset_async(items[i].y_rdo, 0, sizeof(float) * (size_t)items[i].M * (size_t)items[i].hw, stream));
  const EncDesc *dd = reinterpret_cast<const EncDesc *>(ctx->d_ws + o_descs);
  const EncDesc *dd2 = reinterpret_cast<const EncDesc *>(ctx->d_ws + o_descs2);
  const RdoqDesc *dq = reinterpret_cast<const RdoqDesc *>(ctx->d_ws + o_qdescs);
  LAUNCH_TRY(launch_quant_stats(dd, count, M_max, stream));
  for (int i0 = 0, i1; i0 < count; i0 = i1) {
    const double lambda = lambdas[(size_t)i0 * lambda_stride];
    for (i1 = i0 + 1; i1 < count && lambdas[(size_t)i1 * lambda_stride] == lambda;) ++i1;
    LAUNCH_TRY(launch_rdoq(dd + i0, dq + i0, ctx->d_rate_log2, lambda * 0x1p-24, i1 - i0, M_max, hw_max, n_max, linear, mode, vec, clamp != 0, f16, stream));
  }
  LAUNCH_TRY(launch_quant_stats(dd2, count, M_max, stream));
  if (small_bytes) DEV_TRY(dev::copy_async(ctx->h_ws + o_small, ctx->d_ws + o_small, small_bytes, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  // ---- per item, on the host: the census of y_rdo as the compress call will read it (fgmm_encode.cpp side_info), the sums ------
  for (int i = 0; i < count; ++i) {
    fgmm_rdoq_item &it = items[i];
    const RdoqOff &o = off[(size_t)i];
    const unsigned long long *cb = reinterpret_cast<const unsigned long long *>(ctx->h_ws + o.o_before);
    const unsigned long long *ca = reinterpret_cast<const unsigned long long *>(ctx->h_ws + o.o_after);
    const unsigned long long *cc = reinterpret_cast<const unsigned long long *>(ctx->h_ws + o.o_changed);
    (void)census_side_info(ctx, o.census2, it.M, it.hw, it.zero_bitmap, &it.abs_max); // of y_rdo, as the compress call will read it
    uint64_t before = 0, after = 0, changed = 0;
    for (int c = 0; c < it.M; ++c) {
      if (it.chan_bits_q_after) it.chan_bits_q_after[c] = ca[c];
      before += cb[c];
      after += ca[c];
      changed += cc[c];
    }
    it.n_changed = (int64_t)changed;
    it.bits_q_before = before;
    it.bits_q_after = after;
    it.status = FGMM_OK;
  }
  return FGMM_OK;
}

int fgmm::rdoq_check_items(const fgmm_rdoq_item *items, int count) {
  for (int i = 0; i < count; ++i) {
    const fgmm_rdoq_item &s = items[i];
    if (int rc = check_latent_item(i, s.K, s.M, s.hw, s.y, s.params, items[0].params.dtype)) return rc;
    if ((int64_t)s.M * s.hw && !s.y_rdo) return fail(FGMM_ERR_INVALID, "item %d: null tensor / negative size", i);
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(s.y), r0 = reinterpret_cast<uintptr_t>(s.y_rdo);
    const uintptr_t nb = sizeof(float) * (uintptr_t)s.M * (uintptr_t)s.hw; // (y_rdo is zeroed before the census reads y)
    if (nb && y0 < r0 + nb && r0 < y0 + nb) return fail(FGMM_ERR_INVALID, "item %d: y_rdo may not overlap y", i);
  }
  return FGMM_OK;
}

extern "C" {

int fgmm_gmc_rdoq_batch(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, double lambda) {
  if (!(lambda >= 0.0 && lambda < (double)INFINITY)) return fail(FGMM_ERR_INVALID, "lambda = %g: must be finite and >= 0", lambda);
  if (!ctx || count < 0 || (count && !items) || mode < 0 || mode > 2) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = rdoq_check_items(items, count)) return rc;
  if (count == 0) return FGMM_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const int rc = rdoq_run(ctx, (dev::Stream)stream, items, count, mode, clamp_scales, &lambda, 0);
  if (rc != FGMM_OK) {
    (void)dev::stream_sync((dev::Stream)stream); // (nothing of this call may still be writing the workspace the next one reuses)
    for (int i = 0; i < count; ++i) items[i].status = rc;
  }
  return rc;
}

} // extern "C"
