// fgmm_estimate.cpp — the coded size of a batch of latents without coding them (include/flashgmm_amd.h section 3b): what
// fgmm_gmc_compress_batch would return, priced on the GPU.  The encode call's front half - quant_stats_kernel and
// chan_compact_kernel, unchanged - then rate_kernel (fgmm_rate.hip) in place of symtab_kernel: no table is written, nothing but
// the per-channel census and sums (a few KB) crosses PCIe, no host worker runs.  The census is laid out and read by the compress
// call's own helpers (fgmm_encode.cpp).  Also the building block over a finished table, fgmm_symtab_bits_hip.  A file of its own: the
// host sources that build against the fake device reference no launcher of these.
#include "fgmm_ctx.h"

using namespace fgmm;

namespace fgmm {
// the context's device copy of L[r] = round(2^24 * log2 r): uploaded on first use (256 KB), kept until fgmm_ctx_trim
int ensure_rate_table(fgmm_ctx *ctx) {
  if (ctx->d_rate_log2) return FGMM_OK;
  void *p = nullptr;
  DEV_TRY(dev::malloc_device(&p, sizeof(uint32_t) * 65536));
  const int e = dev::copy_sync(p, rate_log2_table(), sizeof(uint32_t) * 65536, dev::kH2D);
  if (e != 0) {
    (void)dev::free_device(p);
    return fail(FGMM_ERR_HIP, "upload of the log2 table -> %s", dev::error_string(e));
  }
  ctx->d_rate_log2 = static_cast<uint32_t *>(p);
  return FGMM_OK;
}

int check_latent_item(int i, int K, int M, int64_t hw, const float *y, const fgmm_params &p, int batch_dtype) {
  if (K != FGMM_K) return fail(FGMM_ERR_INVALID, "K = %d: the reference binds K = 4 only", K);
  if (M < 0 || hw < 0 || ((int64_t)M * hw && (!y || !p.scales || !p.means || !p.weights)))
    return fail(FGMM_ERR_INVALID, "item %d: null tensor / negative size", i);
  if (p.dtype != batch_dtype || (p.dtype != FGMM_F32 && p.dtype != FGMM_F16))
    return fail(FGMM_ERR_INVALID, "item %d: parameter dtype must be FGMM_F32 or FGMM_F16 and the same for a whole batch", i);
  if (p.flags & ~FGMM_PARAMS_LOGITS) return fail(FGMM_ERR_INVALID, "item %d: unknown fgmm_params.flags %d", i, p.flags);
  return FGMM_OK;
}
} // namespace fgmm

namespace {

struct RateOff { // workspace offsets of one item
  CensusOff census;
  size_t o_bits, o_byp;
};

int estimate_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_rate_item *items, int count, int mode, int clamp) {
  int rc;
  if ((rc = ensure_rate_table(ctx))) return rc;
  // ---- workspace: [EncDesc x count][RateDesc x count][small: per item min | max | nz | list | channel bits | channel bypass] ----
  Arena ar;
  const size_t o_descs = ar.take(sizeof(EncDesc) * (size_t)count);
  const size_t o_rdescs = ar.take(sizeof(RateDesc) * (size_t)count);
  const size_t o_small = ar.take(0);
  std::vector<RateOff> off((size_t)count);
  int M_max = 0;
  int64_t hw_max = 0, n_max = 0;
  for (int i = 0; i < count; ++i) {
    const fgmm_rate_item &it = items[i];
    RateOff &o = off[(size_t)i];
    o.census = census_take(ar, it.M);
    o.o_bits = ar.take(sizeof(unsigned long long) * it.M, 16);
    o.o_byp = ar.take(sizeof(unsigned long long) * it.M, 16);
    M_max = std::max(M_max, it.M);
    hw_max = std::max(hw_max, it.hw);
    n_max = std::max(n_max, (int64_t)it.M * it.hw);
  }
  const size_t small_bytes = ar.off - o_small;
  if ((rc = ctx->ensure_device(ar.off)) || (rc = ctx->ensure_host(ar.off)) || (rc = ctx->ensure_events(1))) return rc;
  // ---- descriptors ------------------------------------------------------------------------------------------------------------
  EncDesc *hd = reinterpret_cast<EncDesc *>(ctx->h_ws + o_descs);
  RateDesc *hr = reinterpret_cast<RateDesc *>(ctx->h_ws + o_rdescs);
  const bool f16 = count > 0 && items[0].params.dtype == FGMM_F16;
  bool vec4 = true, linear = true;
  for (int i = 0; i < count; ++i) {
    const fgmm_rate_item &it = items[i];
    const RateOff &o = off[(size_t)i];
    EncDesc &d = hd[i];
    census_desc(d, ctx, o.census, it.y, &it.params, it.M, it.hw, clamp);
    RateDesc &r = hr[i];
    r.chan_bits = reinterpret_cast<unsigned long long *>(ctx->d_ws + o.o_bits);
    r.chan_bypass = reinterpret_cast<unsigned long long *>(ctx->d_ws + o.o_byp);
    r.bits_map = (int64_t)it.M * it.hw ? it.bits_map : nullptr;
    vec4 = vec4 && enc_vec4_ok(d, r.bits_map, f16);
  }
  const int vec = vec4 ? 4 : 1;
  for (int i = 0; i < count; ++i) linear = linear && items[i].hw % (64 * vec) == 0;
  // ---- kernels, the small region back -----------------------------------------------------------------------------------------
  DEV_TRY(dev::copy_async(ctx->d_ws + o_descs, hd, o_small - o_descs, dev::kH2D, stream)); // (both descriptor arrays: one copy)
  DEV_TRY(dev::memset_async(ctx->d_ws + o_small, 0, small_bytes, stream));
  for (int i = 0; i < count; ++i) // the map is zero in the channels that are not coded; rate_kernel writes the others
    if (hr[i].bits_map) DEV_TRY(dev::memset_async(hr[i].bits_map, 0, sizeof(float) * (size_t)items[i].M * (size_t)items[i].hw, stream));
  const EncDesc *dd = reinterpret_cast<const EncDesc *>(ctx->d_ws + o_descs);
  const RateDesc *dr = reinterpret_cast<const RateDesc *>(ctx->d_ws + o_rdescs);
  LAUNCH_TRY(launch_quant_stats(dd, count, M_max, stream));
  LAUNCH_TRY(launch_rate(dd, dr, ctx->d_rate_log2, count, M_max, hw_max, n_max, linear, mode, vec, clamp != 0, f16, stream));
  if (small_bytes) DEV_TRY(dev::copy_async(ctx->h_ws + o_small, ctx->d_ws + o_small, small_bytes, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  // ---- per item, on the host: the census as the compress call reads it (fgmm_encode.cpp side_info), the sums --------------------
  for (int i = 0; i < count; ++i) {
    fgmm_rate_item &it = items[i];
    const RateOff &o = off[(size_t)i];
    const unsigned long long *cb = reinterpret_cast<const unsigned long long *>(ctx->h_ws + o.o_bits);
    const unsigned long long *cy = reinterpret_cast<const unsigned long long *>(ctx->h_ws + o.o_byp);
    const int n_nz = census_side_info(ctx, o.census, it.M, it.hw, it.zero_bitmap, &it.abs_max);
    uint64_t bits = 0, byp = 0;
    for (int c = 0; c < it.M; ++c) {
      if (it.chan_bits_q) it.chan_bits_q[c] = cb[c];
      bits += cb[c];
      byp += cy[c];
    }
    it.n_symbols = (int64_t)n_nz * it.hw;
    it.n_bypass = (int64_t)byp;
    it.bits_q = bits;
    it.bytes_pred = rate_stream_bytes(bits);
    it.status = FGMM_OK;
  }
  return FGMM_OK;
}

} // namespace

extern "C" {

int fgmm_gmc_estimate_batch(fgmm_ctx *ctx, void *stream, fgmm_rate_item *items, int count, int mode, int clamp_scales) {
  if (!ctx || count < 0 || (count && !items) || mode < 0 || mode > 2) return fail(FGMM_ERR_INVALID, "bad argument");
  for (int i = 0; i < count; ++i) {
    const fgmm_rate_item &s = items[i];
    if (int rc = check_latent_item(i, s.K, s.M, s.hw, s.y, s.params, items[0].params.dtype)) return rc;
  }
  if (count == 0) return FGMM_OK;
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const int rc = estimate_batch(ctx, (dev::Stream)stream, items, count, mode, clamp_scales);
  if (rc != FGMM_OK) {
    (void)dev::stream_sync((dev::Stream)stream); // (nothing of this call may still be writing the workspace the next one reuses)
    for (int i = 0; i < count; ++i) items[i].status = rc;
  }
  return rc;
}

int fgmm_symtab_bits_hip(fgmm_ctx *ctx, void *stream, const uint32_t *packed, const int32_t *symbols_or_null, int64_t n,
                         uint32_t *cost_q_or_null, uint64_t *bits_q_dev, uint64_t *n_bypass_dev) {
  if (!ctx || n < 0 || (n > 0 && !packed)) return fail(FGMM_ERR_INVALID, "bad argument");
  std::lock_guard<std::mutex> lock(ctx->mu);
  DeviceGuard g(ctx->device);
  if (!g.ok) return fail(FGMM_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  int rc;
  if ((rc = ensure_rate_table(ctx))) return rc;
  dev::Stream s = (dev::Stream)stream;
  if (bits_q_dev) DEV_TRY(dev::memset_async(bits_q_dev, 0, sizeof(uint64_t), s));
  if (n_bypass_dev) DEV_TRY(dev::memset_async(n_bypass_dev, 0, sizeof(uint64_t), s));
  LAUNCH_TRY(launch_symtab_bits(packed, symbols_or_null, n, ctx->d_rate_log2, cost_q_or_null, reinterpret_cast<unsigned long long *>(bits_q_dev),
                                reinterpret_cast<unsigned long long *>(n_bypass_dev), s));
  DEV_TRY(dev::stream_sync(s));
  return FGMM_OK;
}

} // extern "C"
