#!/usr/bin/env python3
"""rd_budget_time.py - what the rate-distortion curve and quantisation to a byte budget cost, on the Kodak batch of bench.py's synthetic
generator (48 streams of [1, 192, 32, 24]; tests/synth.make_latent - NOT real images' latents: no trained checkpoint exists offline).
HIP events on the launch's stream around each call, after warm-up, all in one run:

  curve16_call    ``rd_curve_batch`` at 16 lambdas: census + ONE rdcurve_kernel pass + the fold + a few KB back
  rdoq_call       ``quantize_rdo_batch`` at one lambda: census + ONE rdoq_kernel pass + the census of the result + a few KB back
  budget_call     ``quantize_to_budget_batch`` at refine = 2, every stream its own group, the budget half way between the predicted bytes
                  at lambda = 0 and at lambda = 16: census + three rdcurve_kernel passes + the RDOQ path at the lambdas found
  rdoq_x48        48 ``quantize_rdo_batch`` calls: the same 3 x 16 evaluations done the only way possible without the curve
  *_w             the first three with the weighted distortion of header section 3e: a shared ``channel_weights`` [M] cycling 0.25, 1, 4 and
                  a ``position_weights`` [N, 1, h, w] cycling 0.5, 1, 2, 1 (the weighted instantiations of the two kernels, the domain
                  check beside the census); the budgets are those of the unweighted rows

The kernels alone (rdcurve_kernel against rdoq_kernel): run this script under
``rocprofv3 --kernel-trace --stats -- python scripts/rd_budget_time.py --reps 20`` and read the kernel rows.
``--no-x48`` leaves the 48-call row out.  Prints one JSON object; profiles/rd_budget.md and profiles/rdo_weights.md record runs."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", default="polya")
    ap.add_argument("--no-x48", action="store_true")
    a = ap.parse_args()
    import bench
    from flashgmm_amd import GaussianMixtureConditional
    from rdoq_time import timed

    dev = torch.device("cuda:0")
    _, devt, _ = bench.make_workload(0, a.images, dev, "kodak24", keep_host_images=0)
    y, s, m, w = (torch.cat([st[k] for st in devt]) for k in range(4))  # stacked [N, ...]
    gmc = GaussianMixtureConditional(K=4, mode=a.mode)
    lams = [0.0] + [16.0 * 2.0 ** (j - 15) for j in range(1, 16)]
    c = gmc.rd_curve_batch(y, s, m, w, [0.0, 16.0])
    budgets = [((r.nbytes[0] + r.nbytes[1]) // 2) // 4 * 4 for r in c]
    out = {"workload": f"kodak24 synthetic, {a.images} images, {y.shape[0]} streams, {y.numel()} latents", "mode": a.mode}
    out["curve16_call"] = timed(lambda: gmc.rd_curve_batch(y, s, m, w, lams), a.reps, a.warmup)
    out["rdoq_call"] = timed(lambda: gmc.quantize_rdo_batch(y, s, m, w, 0.1), a.reps, a.warmup)
    out["budget_call"] = timed(lambda: gmc.quantize_to_budget_batch(y, s, m, w, budgets, refine=2), a.reps, a.warmup)
    N, M, h, wd = y.shape
    kw = {"channel_weights": torch.tensor([(0.25, 1.0, 4.0)[c % 3] for c in range(M)], device=dev),
          "position_weights": torch.tensor([(0.5, 1.0, 2.0, 1.0)[p % 4] for p in range(h * wd)], device=dev).view(1, 1, h, wd).repeat(N, 1, 1, 1)}
    out["curve16_call_w"] = timed(lambda: gmc.rd_curve_batch(y, s, m, w, lams, **kw), a.reps, a.warmup)
    out["rdoq_call_w"] = timed(lambda: gmc.quantize_rdo_batch(y, s, m, w, 0.1, **kw), a.reps, a.warmup)
    out["budget_call_w"] = timed(lambda: gmc.quantize_to_budget_batch(y, s, m, w, budgets, refine=2, **kw), a.reps, a.warmup)
    out["weighted_to_unweighted"] = {k: round(out[k + "_w"]["median_ms"] / out[k]["median_ms"], 3) for k in ("curve16_call", "rdoq_call", "budget_call")}
    rows = ["curve16_call", "budget_call"]
    if not a.no_x48:
        out["rdoq_x48"] = timed(lambda: [gmc.quantize_rdo_batch(y, s, m, w, 0.01 * (k + 1)) for k in range(48)], max(a.reps // 6, 3), 1)
        rows.append("rdoq_x48")
    r = out["rdoq_call"]["median_ms"]
    out["ratios_to_rdoq_call"] = {k: round(out[k]["median_ms"] / r, 3) for k in rows}
    q = gmc.quantize_to_budget_batch(y, s, m, w, budgets, refine=2)
    out["budget"] = {"bytes_at_0": sum(r.nbytes[0] for r in c), "bytes_at_16": sum(r.nbytes[1] for r in c), "budget": sum(budgets),
                     "bytes_pred": sum(r.bytes_pred for r in q), "met": sum(r.budget_met for r in q), "passes": sorted({r.passes for r in q}),
                     "lambda_min": min(r.lam for r in q), "lambda_max": max(r.lam for r in q)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
