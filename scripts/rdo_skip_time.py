#!/usr/bin/env python3
"""rdo_skip_time.py - what channel skipping (include/flashgmm_amd.h section 3f) costs and buys, on the Kodak batch of bench.py's synthetic
generator (48 streams of [1, 192, 32, 24]; tests/synth.make_latent - NOT real images' latents: no trained checkpoint exists offline).
HIP events on the launch's stream around each call (scripts/rdoq_time.py: timed), after warm-up, all in one run:

  rdoq_call       ``quantize_rdo_batch`` at lambda = 0.5 through the per-item boundary (a list of 48 items: the path the skip form takes too)
  curve16_call    ``rd_curve_batch`` at 16 lambdas
  budget_call     ``quantize_to_budget_batch`` at refine = 2, every stream its own group, the budget half way between the predicted bytes
                  at lambda = 0 and at lambda = 16 of the plain curve
  *_skip          the same three with ``channel_skip=True`` (``--skip``; a build without section 3f runs the first three only, so the
                  same script times the parent commit)
  rd              ``--skip``: per lambda in {0.1, 0.5, 2} the predicted bytes, the weighted added distortion (``ddist_q`` * 2^-32, summed over
                  the batch) and the latents changed with and without skipping, the channels skipped and the coded channels

The kernels alone: run under ``rocprofv3 --kernel-trace --stats -- python scripts/rdo_skip_time.py --skip --reps 20 --no-rd`` and read the
kernel rows.  Prints one JSON object; profiles/rdo_skip.md records runs."""
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
    ap.add_argument("--skip", action="store_true", help="also the channel_skip=True forms")
    ap.add_argument("--no-rd", action="store_true", help="timing only (profiler runs)")
    a = ap.parse_args()
    import bench
    from flashgmm_amd import GaussianMixtureConditional
    from rdoq_time import timed

    dev = torch.device("cuda:0")
    _, devt, _ = bench.make_workload(0, a.images, dev, "kodak24", keep_host_images=0)
    ys, ss, ms, ws = ([st[k] for st in devt] for k in range(4))  # sequences: the per-item boundary
    gmc = GaussianMixtureConditional(K=4, mode=a.mode)
    lams = [0.0] + [16.0 * 2.0 ** (j - 15) for j in range(1, 16)]
    c = gmc.rd_curve_batch(ys, ss, ms, ws, [0.0, 16.0])
    budgets = [((r.nbytes[0] + r.nbytes[1]) // 2) // 4 * 4 for r in c]
    out = {"workload": f"kodak24 synthetic, {a.images} images, {len(ys)} streams, {sum(y.numel() for y in ys)} latents", "mode": a.mode}
    forms = [("", {})] + ([("_skip", {"channel_skip": True})] if a.skip else [])
    for tag, kw in forms:
        out["rdoq_call" + tag] = timed(lambda: gmc.quantize_rdo_batch(ys, ss, ms, ws, 0.5, **kw), a.reps, a.warmup)
        out["curve16_call" + tag] = timed(lambda: gmc.rd_curve_batch(ys, ss, ms, ws, lams, **kw), a.reps, a.warmup)
        out["budget_call" + tag] = timed(lambda: gmc.quantize_to_budget_batch(ys, ss, ms, ws, budgets, refine=2, **kw), a.reps, a.warmup)
    if a.skip:
        out["skip_to_plain"] = {k: round(out[k + "_skip"]["median_ms"] / out[k]["median_ms"], 3) for k in ("rdoq_call", "curve16_call", "budget_call")}
    if a.skip and not a.no_rd:
        rd = {}
        for lam in (0.1, 0.5, 2.0):
            plain = gmc.rd_curve_batch(ys, ss, ms, ws, [lam])
            skip = gmc.rd_curve_batch(ys, ss, ms, ws, [lam], channel_skip=True)
            q = gmc.quantize_rdo_batch(ys, ss, ms, ws, lam, channel_skip=True)
            assert [(r.bits_q_after, r.n_changed, r.ddist_q, r.n_skipped) for r in q] == [(r.bits_q_after[0], r.n_changed[0], r.ddist_q[0], r.n_skipped[0]) for r in skip]
            coded = sum(r.n_symbols // ys[0][0, 0].numel() for r in plain)
            rd[str(lam)] = {"bytes_pred": sum(r.nbytes[0] for r in plain), "bytes_pred_skip": sum(r.nbytes[0] for r in skip),
                            "dist_added": sum(r.distortion_added[0] for r in plain), "dist_added_skip": sum(r.distortion_added[0] for r in skip),
                            "n_changed": sum(r.n_changed[0] for r in plain), "n_changed_skip": sum(r.n_changed[0] for r in skip),
                            "channels_skipped": sum(r.n_skipped[0] for r in skip), "channels_eligible": sum(r.n_eligible for r in q), "channels_coded": coded}
        out["bytes_at_0"] = sum(r.nbytes[0] for r in c)
        out["rd"] = rd
        b0 = gmc.quantize_to_budget_batch(ys, ss, ms, ws, budgets, refine=2)
        b1 = gmc.quantize_to_budget_batch(ys, ss, ms, ws, budgets, refine=2, channel_skip=True)
        out["budget"] = {"budget": sum(budgets), "bytes_pred": sum(r.bytes_pred for r in b0), "bytes_pred_skip": sum(r.bytes_pred for r in b1),
                         "lambda_mean": sum(r.lam for r in b0) / len(b0), "lambda_mean_skip": sum(r.lam for r in b1) / len(b1),
                         "met": sum(r.budget_met for r in b0), "met_skip": sum(r.budget_met for r in b1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
