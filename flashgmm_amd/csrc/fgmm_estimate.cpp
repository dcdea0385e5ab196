// fgmm_estimate.cpp — the coded size of a batch of latents without coding them (include/flashgmm_amd.h section 3b): what
// fgmm_gmc_compress_batch would return, priced on the GPU.  The encode call's front half - quant_stats_kernel and
// chan_compact_kernel, unchanged - then rate_kernel (fgmm_rate.hip) in place of symtab_kernel: no table is written, nothing but
// the per-channel census and sums (a few KB) crosses PCIe, no host worker runs.  That front half is common to the four calls that
// price latents - this one, RDOQ (fgmm_rdoq.cpp), the curve and the budget call (fgmm_rdcurve.cpp) - and stands here ONCE, with their
// item validation: the frame declared in fgmm_ctx.h.  The census is laid out and read by the compress call's own helpers
// (fgmm_encode.cpp).  Also the building block over a finished table, fgmm_symtab_bits_hip.  A file of its own: the host sources that
// build against the fake device reference no launcher of these.
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

int check_latent_items(const std::vector<LatentIn> &in) {
  for (int i = 0; i < (int)in.size(); ++i) {
    const LatentIn &s = in[(size_t)i];
    const fgmm_params &p = *s.params;
    if (s.K != FGMM_K) return fail(FGMM_ERR_INVALID, "K = %d: the reference binds K = 4 only", s.K);
    if (s.M < 0 || s.hw < 0 || ((int64_t)s.M * s.hw && (!s.y || !p.scales || !p.means || !p.weights)))
      return fail(FGMM_ERR_INVALID, "item %d: null tensor / negative size", i);
    if (p.dtype != in[0].params->dtype || (p.dtype != FGMM_F32 && !planes_two_byte(p.dtype)))
      return fail(FGMM_ERR_INVALID, "item %d: parameter dtype must be FGMM_F32, FGMM_F16 or FGMM_BF16 and the same for a whole batch", i);
    if (p.flags & ~FGMM_PARAMS_LOGITS) return fail(FGMM_ERR_INVALID, "item %d: unknown fgmm_params.flags %d", i, p.flags);
  }
  return FGMM_OK;
}

int LatentFrame::layout(const LatentNeeds &n) {
  int rc;
  if ((rc = ensure_rate_table(ctx))) return rc;
  census2 = n.census2;
  Arena ar;
  o_descs = ar.take(sizeof(EncDesc) * (size_t)count * (census2 ? 2 : 1));
  o_call = ar.take(n.desc_bytes * (size_t)count);
  for (int i = 0; w && i < count; ++i) weighted = weighted || w[i].chan_w || w[i].pos_w;
  if (weighted) o_wdesc = ar.take(sizeof(RdoWDesc) * (size_t)count);
  o_small = ar.take(0);
  if (weighted) o_wbad = ar.take(sizeof(uint32_t) * (size_t)count);
  census.resize((size_t)count), census_out.resize((size_t)count), o_back.resize((size_t)count), o_acc.resize((size_t)count);
  out.assign((size_t)count, nullptr);
  for (int i = 0; i < count; ++i) {
    const LatentIn &it = in[(size_t)i];
    census[(size_t)i] = census_take(ar, it.M);
    if (census2) census_out[(size_t)i] = census_take(ar, it.M);
    M_max = std::max(M_max, it.M);
    hw_max = std::max(hw_max, it.hw);
    n_max = std::max(n_max, (int64_t)it.M * it.hw);
  }
  o_sums = ar.take(0, 16);
  for (int i = 0; i < count; ++i) o_back[(size_t)i] = ar.take(sizeof(uint64_t) * (n.back_item + n.back_chan * (size_t)in[(size_t)i].M), 16);
  o_dev = ar.take(0, 16);
  for (int i = 0; i < count; ++i) o_acc[(size_t)i] = ar.take(sizeof(uint64_t) * n.dev_chan * (size_t)in[(size_t)i].M, 16);
  end = ar.off;
  if ((rc = ctx->ensure_device(end)) || (rc = ctx->ensure_host(o_dev)) || (rc = ctx->ensure_events(1))) return rc;
  planes = in[0].params->dtype;
  for (int i = 0; i < count; ++i) {
    const LatentIn &it = in[(size_t)i];
    census_desc(ws<EncDesc>(ctx->h_ws, o_descs)[i], ctx, census[(size_t)i], it.y, it.params, it.M, it.hw, clamp);
  }
  return FGMM_OK;
}

int LatentFrame::start() {
  EncDesc *hd = ws<EncDesc>(ctx->h_ws, o_descs);
  bool vec4 = true;
  for (int i = 0; i < count; ++i) {
    const LatentIn &it = in[(size_t)i];
    if (census2) census_desc(hd[count + i], ctx, census_out[(size_t)i], out[(size_t)i], nullptr, it.M, it.hw, clamp);
    vec4 = vec4 && enc_vec4_ok(hd[i], out[(size_t)i], planes_two_byte(planes));
    if (weighted) { // pos_w is read VEC positions wide as the planes are (hw % 4 is enc_vec4_ok's)
      ws<RdoWDesc>(ctx->h_ws, o_wdesc)[i] = RdoWDesc{w[i].chan_w, w[i].pos_w};
      vec4 = vec4 && (reinterpret_cast<uintptr_t>(w[i].pos_w) & 15) == 0;
    }
  }
  vec = vec4 ? 4 : 1;
  for (const LatentIn &it : in) linear = linear && it.hw % (64 * vec) == 0;
  DEV_TRY(dev::copy_async(ctx->d_ws + o_descs, hd, o_small - o_descs, dev::kH2D, stream)); // (every descriptor array: one copy)
  DEV_TRY(dev::memset_async(ctx->d_ws + o_small, 0, o_dev - o_small, stream));
  for (int i = 0; i < count; ++i) { // zero in the channels that are not coded; the call's kernel writes the others
    const size_t n = (size_t)in[(size_t)i].M * (size_t)in[(size_t)i].hw;
    if (out[(size_t)i] && n) DEV_TRY(dev::memset_async(out[(size_t)i], 0, sizeof(float) * n, stream));
  }
  LAUNCH_TRY(launch_quant_stats(dd(), count, M_max, stream));
  if (weighted && w_check)
    LAUNCH_TRY(launch_rdo_weights_check(dd(), ws<const RdoWDesc>(ctx->d_ws, o_wdesc), ws<uint32_t>(ctx->d_ws, o_wbad), count, M_max, hw_max, stream));
  return FGMM_OK;
}

int LatentFrame::finish(size_t from) {
  if (census2) LAUNCH_TRY(launch_quant_stats(dd(true), count, M_max, stream));
  if (o_dev > from) DEV_TRY(dev::copy_async(ctx->h_ws + from, ctx->d_ws + from, o_dev - from, dev::kD2H, stream));
  DEV_TRY(dev::event_record(ctx->events[0], stream));
  DEV_TRY(dev::event_sync(ctx->events[0]));
  if (weighted && w_check && !w_checked && from <= o_wbad) {
    w_checked = true;
    for (int i = 0; i < count; ++i)
      if (ws<const uint32_t>(ctx->h_ws, o_wbad)[i])
        return fail(FGMM_ERR_INVALID, "item %d: a factor of chan_w / pos_w is not finite or lies outside [0, %g]", i, (double)FGMM_RDO_W_MAX);
  }
  return FGMM_OK;
}
} // namespace fgmm

namespace {

int estimate_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_rate_item *items, int count, int mode, int clamp) {
  LatentFrame fr(ctx, stream, latent_in(items, count), clamp);
  int rc;
  if ((rc = fr.layout({sizeof(RateDesc), 0, 2, 0, false}))) return rc; // per channel: its bits | its bypass symbols
  RateDesc *hr = ws<RateDesc>(ctx->h_ws, fr.o_call);
  for (int i = 0; i < count; ++i) {
    hr[i].chan_bits = ws<unsigned long long>(ctx->d_ws, fr.o_back[(size_t)i]);
    hr[i].chan_bypass = hr[i].chan_bits + items[i].M;
    hr[i].bits_map = fr.out[(size_t)i] = (int64_t)items[i].M * items[i].hw ? items[i].bits_map : nullptr;
  }
  if ((rc = fr.start())) return rc;
  LAUNCH_TRY(launch_rate(fr.dd(), ws<const RateDesc>(ctx->d_ws, fr.o_call), ctx->d_rate_log2, count, fr.M_max, fr.hw_max, fr.n_max, fr.linear, mode,
                         fr.vec, clamp != 0, fr.planes, stream));
  if ((rc = fr.finish(fr.o_small))) return rc;
  // ---- per item, on the host: the census as the compress call reads it (fgmm_encode.cpp side_info), the sums --------------------
  for (int i = 0; i < count; ++i) {
    fgmm_rate_item &it = items[i];
    const uint64_t *cb = ws<const uint64_t>(ctx->h_ws, fr.o_back[(size_t)i]), *cy = cb + it.M;
    const int n_nz = census_side_info(ctx, fr.census[(size_t)i], it.M, it.hw, it.zero_bitmap, &it.abs_max);
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
  if (int rc = check_latent_items(latent_in(items, count))) return rc;
  return latent_call(ctx, stream, items, count, [&](dev::Stream s) { return estimate_batch(ctx, s, items, count, mode, clamp_scales); });
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
