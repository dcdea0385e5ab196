// fgmm_rdcurve.cpp — the rate-distortion curve of a batch of latents and their quantisation to a byte budget (include/flashgmm_amd.h
// sections 3d, 3e and 3f).  The frame of fgmm_estimate.cpp once per call (LatentFrame: quant_stats_kernel and chan_compact_kernel give the
// channels the compress call would code for y), then one or more PASSES: rdcurve_kernel (fgmm_rdcurve.hip) at up to 16 lambdas per
// item, the channels' sums folded to the items' on the device, a few KB back.  The budget call searches lambda on those passes by the
// header's rule, every group on its own grid within one launch, and ends in the RDOQ call's own path (fgmm_rdoq.cpp: rdoq_run) at the
// lambdas found.  A file of its own, as fgmm_rdoq.cpp: the host sources that build against the fake device reference no launcher of these.
#include <algorithm>
#include <cmath>

#include "fgmm_ctx.h"

using namespace fgmm;

namespace {

struct Curve : LatentFrame { // the passes of a call, on the frame: a pass sets n_lambda and lam_q of every item in `hc`, then run()
  using LatentFrame::LatentFrame;
  RdCurveDesc *hc = nullptr; // host copy of the curve descriptors
  bool census_back = false;
  bool skip = false; // section 3f: the kernels' skip forms, on their wider rows
  const uint64_t *sums(int i) const { return ws<const uint64_t>(ctx->h_ws, o_back[(size_t)i]); }

  int begin() { // the census, once: every pass prices the channels it names
    // the item's row of sums | on the device, a row per channel
    if (int rc = layout({sizeof(RdCurveDesc), (size_t)(skip ? kRdCurveSumsS : kRdCurveRow), 0, (size_t)(skip ? kRdCurveRowS : kRdCurveRow), false})) return rc;
    hc = ws<RdCurveDesc>(ctx->h_ws, o_call);
    for (int i = 0; i < count; ++i) {
      memset(&hc[i], 0, sizeof hc[i]);
      hc[i].chan_acc = ws<unsigned long long>(ctx->d_ws, o_acc[(size_t)i]);
      hc[i].sums = ws<unsigned long long>(ctx->d_ws, o_back[(size_t)i]);
      hc[i].chan_w = chan_w(i), hc[i].pos_w = pos_w(i);
    }
    return start();
  }

  // one pass: only the curve descriptors go up again; back come the items' sums and, after the first pass alone, the census
  int run(int mode) {
    DEV_TRY(dev::copy_async(ctx->d_ws + o_call, hc, sizeof(RdCurveDesc) * (size_t)count, dev::kH2D, stream));
    DEV_TRY(dev::memset_async(ctx->d_ws + o_sums, 0, end - o_sums, stream)); // the items' sums and the channels'
    LAUNCH_TRY(launch_rdcurve(dd(), ws<const RdCurveDesc>(ctx->d_ws, o_call), ctx->d_rate_log2, weighted, skip, count, M_max, hw_max, n_max, linear, mode,
                              vec, clamp != 0, planes, stream));
    const size_t from = census_back ? o_sums : o_small;
    census_back = true;
    return finish(from);
  }
};

bool lambda_ok(double v) { return v >= 0.0 && v < (double)INFINITY; } // (false for NaN)

int curve_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_rdcurve_item *items, int count, int mode, int clamp, const double *lambdas, int n_lambda,
                const fgmm_rdo_weights *w, fgmm_rdcurve_skip *sk) {
  Curve cv(ctx, stream, latent_in(items, count), clamp);
  cv.w = w, cv.skip = sk != nullptr;
  int rc;
  if ((rc = cv.begin())) return rc;
  for (int i = 0; i < count; ++i) {
    cv.hc[i].n_lambda = n_lambda;
    for (int j = 0; j < n_lambda; ++j) cv.hc[i].lam_q[j] = lambdas[j] * 0x1p-24;
  }
  if ((rc = cv.run(mode))) return rc;
  for (int i = 0; i < count; ++i) {
    fgmm_rdcurve_item &it = items[i];
    const uint64_t *s = cv.sums(i);
    int32_t abs_max;
    const int n_nz = census_side_info(ctx, cv.census[(size_t)i], it.M, it.hw, nullptr, &abs_max);
    it.bits_q_before = s[0];
    for (int j = 0; j < n_lambda; ++j) {
      it.bits_q_after[j] = s[1 + j];
      it.n_changed[j] = s[1 + FGMM_RDCURVE_MAX + j];
      it.ddist_q[j] = s[1 + 2 * FGMM_RDCURVE_MAX + j];
      if (sk) sk[i].n_skipped[j] = s[kRdCurveRow + j];
    }
    if (sk) sk[i].n_eligible = (int64_t)s[kRdCurveRow + FGMM_RDCURVE_MAX];
    it.n_symbols = (int64_t)n_nz * it.hw;
    it.status = FGMM_OK;
  }
  return FGMM_OK;
}

struct Search { // one group's search (header section 3d)
  double grid[FGMM_RDCURVE_MAX];
  double lo = 0.0, hi = 0.0;
  uint64_t f_hi = 0;
  int passes = 0, status = FGMM_OK;
  bool active = true;
};

int budget_batch(fgmm_ctx *ctx, dev::Stream stream, fgmm_rdoq_item *items, int count, int mode, int clamp, const int32_t *group, int n_groups,
                 const uint64_t *budget, double lambda_max, int refine, fgmm_budget_result *results, const fgmm_rdo_weights *w, fgmm_rdo_skip *sk) {
  Curve cv(ctx, stream, latent_in(items, count), clamp);
  cv.w = w, cv.skip = sk != nullptr;
  int rc;
  if ((rc = cv.begin())) return rc;
  std::vector<Search> gs((size_t)n_groups);
  for (Search &g : gs) { // round 0: 0, then lambda_max * 2^(j - 15)
    g.grid[0] = 0.0;
    for (int j = 1; j < FGMM_RDCURVE_MAX; ++j) g.grid[j] = lambda_max * ldexp(1.0, j - 15);
  }
  std::vector<uint64_t> f((size_t)n_groups * FGMM_RDCURVE_MAX);
  for (int round = 0; round <= refine; ++round) {
    bool any = false;
    for (const Search &g : gs) any = any || g.active;
    if (!any) break;
    for (int i = 0; i < count; ++i) {
      const Search &g = gs[(size_t)(group ? group[i] : i)];
      cv.hc[i].n_lambda = g.active ? FGMM_RDCURVE_MAX : 0;
      for (int j = 0; j < FGMM_RDCURVE_MAX; ++j) cv.hc[i].lam_q[j] = g.grid[j] * 0x1p-24;
    }
    if ((rc = cv.run(mode))) return rc;
    std::fill(f.begin(), f.end(), 0);
    for (int i = 0; i < count; ++i) {
      const int gi = group ? group[i] : i;
      if (!gs[(size_t)gi].active) continue;
      const uint64_t *s = cv.sums(i);
      for (int j = 0; j < FGMM_RDCURVE_MAX; ++j) f[(size_t)gi * FGMM_RDCURVE_MAX + j] += rate_stream_bytes(s[1 + j]);
    }
    for (int gi = 0; gi < n_groups; ++gi) {
      Search &g = gs[(size_t)gi];
      if (!g.active) continue;
      const uint64_t *fg = &f[(size_t)gi * FGMM_RDCURVE_MAX];
      g.passes++;
      int k = 0;
      while (k < FGMM_RDCURVE_MAX && fg[k] > budget[gi]) ++k; // the first feasible point of the grid
      if (round == 0) {
        if (k == FGMM_RDCURVE_MAX) { // no lambda up to lambda_max fits
          g.hi = lambda_max, g.f_hi = fg[FGMM_RDCURVE_MAX - 1], g.status = FGMM_BUDGET_UNMET, g.active = false;
          continue;
        }
        g.hi = g.grid[k], g.f_hi = fg[k];
        if (k == 0) { // round(y) already fits
          g.active = false;
          continue;
        }
        g.lo = g.grid[k - 1];
      } else {
        if (fg[FGMM_RDCURVE_MAX - 1] > budget[gi]) { // hi, evaluated again, no longer fits: lo and hi stay
          g.active = false;
          continue;
        }
        if (k > 0) g.lo = g.grid[k - 1];
        g.hi = g.grid[k], g.f_hi = fg[k];
      }
      if (round == refine || g.lo == g.hi) {
        g.active = false;
        continue;
      }
      for (int q = 1; q < FGMM_RDCURVE_MAX; ++q) g.grid[q - 1] = g.lo + (g.hi - g.lo) * (double)q / 16.0;
      g.grid[FGMM_RDCURVE_MAX - 1] = g.hi;
    }
  }
  // 3c at the lambdas found: the RDOQ call's own path, its second census included (the workspace of the passes is no longer needed)
  std::vector<double> lam((size_t)count);
  for (int i = 0; i < count; ++i) lam[(size_t)i] = gs[(size_t)(group ? group[i] : i)].hi;
  if ((rc = rdoq_run(ctx, stream, items, count, mode, clamp, lam.data(), 1, w, false, sk))) return rc; // (the factors' domain: checked by the first pass)
  for (int gi = 0; gi < n_groups; ++gi) {
    const Search &g = gs[(size_t)gi];
    results[gi].lambda = g.hi;
    results[gi].bytes_pred = g.f_hi;
    results[gi].passes = g.passes;
    results[gi].status = g.status;
  }
  return FGMM_OK;
}

} // namespace

extern "C" {

int fgmm_gmc_rdcurve_batch_s(fgmm_ctx *ctx, void *stream, fgmm_rdcurve_item *items, int count, int mode, int clamp_scales, const double *lambdas,
                             int n_lambda, const fgmm_rdo_weights *w, fgmm_rdcurve_skip *skip) {
  if (n_lambda < 1 || n_lambda > FGMM_RDCURVE_MAX || !lambdas)
    return fail(FGMM_ERR_INVALID, "n_lambda = %d: must lie in 1 .. %d", n_lambda, FGMM_RDCURVE_MAX);
  for (int j = 0; j < n_lambda; ++j)
    if (!lambda_ok(lambdas[j])) return fail(FGMM_ERR_INVALID, "lambda[%d] = %g: must be finite and >= 0", j, lambdas[j]);
  if (!ctx || count < 0 || (count && !items) || mode < 0 || mode > 2) return fail(FGMM_ERR_INVALID, "bad argument");
  if (int rc = check_latent_items(latent_in(items, count))) return rc;
  return latent_call(ctx, stream, items, count, [&](dev::Stream s) { return curve_batch(ctx, s, items, count, mode, clamp_scales, lambdas, n_lambda, w, skip); });
}
int fgmm_gmc_rdcurve_batch_w(fgmm_ctx *ctx, void *stream, fgmm_rdcurve_item *items, int count, int mode, int clamp_scales, const double *lambdas,
                             int n_lambda, const fgmm_rdo_weights *w) {
  return fgmm_gmc_rdcurve_batch_s(ctx, stream, items, count, mode, clamp_scales, lambdas, n_lambda, w, nullptr);
}
int fgmm_gmc_rdcurve_batch(fgmm_ctx *ctx, void *stream, fgmm_rdcurve_item *items, int count, int mode, int clamp_scales, const double *lambdas,
                           int n_lambda) {
  return fgmm_gmc_rdcurve_batch_w(ctx, stream, items, count, mode, clamp_scales, lambdas, n_lambda, nullptr);
}

int fgmm_gmc_rdoq_budget_batch_s(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, const int32_t *group,
                                 int n_groups, const uint64_t *budget_bytes, double lambda_max, int refine, fgmm_budget_result *results,
                                 const fgmm_rdo_weights *w, fgmm_rdo_skip *skip) {
  if (!(lambda_max > 0.0 && lambda_max < (double)INFINITY)) return fail(FGMM_ERR_INVALID, "lambda_max = %g: must be finite and > 0", lambda_max);
  if (refine < 0 || refine > 8) return fail(FGMM_ERR_INVALID, "refine = %d: must lie in 0 .. 8", refine);
  if (!ctx || count < 0 || (count && !items) || mode < 0 || mode > 2 || n_groups < 0 || (n_groups && (!budget_bytes || !results)))
    return fail(FGMM_ERR_INVALID, "bad argument");
  if (!group && n_groups != count) return fail(FGMM_ERR_INVALID, "n_groups = %d: without group ids every item is its own group (%d)", n_groups, count);
  if (group) {
    std::vector<char> seen((size_t)n_groups, 0);
    for (int i = 0; i < count; ++i) {
      if (group[i] < 0 || group[i] >= n_groups) return fail(FGMM_ERR_INVALID, "item %d: group %d outside 0 .. %d", i, group[i], n_groups - 1);
      seen[(size_t)group[i]] = 1;
    }
    for (int gi = 0; gi < n_groups; ++gi)
      if (!seen[(size_t)gi]) return fail(FGMM_ERR_INVALID, "group %d is empty", gi);
  }
  if (int rc = rdoq_check_items(items, count)) return rc;
  return latent_call(ctx, stream, items, count, [&](dev::Stream s) {
    return budget_batch(ctx, s, items, count, mode, clamp_scales, group, n_groups, budget_bytes, lambda_max, refine, results, w, skip);
  });
}
int fgmm_gmc_rdoq_budget_batch_w(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, const int32_t *group,
                                 int n_groups, const uint64_t *budget_bytes, double lambda_max, int refine, fgmm_budget_result *results,
                                 const fgmm_rdo_weights *w) {
  return fgmm_gmc_rdoq_budget_batch_s(ctx, stream, items, count, mode, clamp_scales, group, n_groups, budget_bytes, lambda_max, refine, results, w, nullptr);
}
int fgmm_gmc_rdoq_budget_batch(fgmm_ctx *ctx, void *stream, fgmm_rdoq_item *items, int count, int mode, int clamp_scales, const int32_t *group,
                               int n_groups, const uint64_t *budget_bytes, double lambda_max, int refine, fgmm_budget_result *results) {
  return fgmm_gmc_rdoq_budget_batch_w(ctx, stream, items, count, mode, clamp_scales, group, n_groups, budget_bytes, lambda_max, refine, results, nullptr);
}

} // extern "C"
