#!/usr/bin/env python3
"""rdoq_time.py - what rate-distortion optimised quantisation costs and buys, on the Kodak batch of bench.py's synthetic generator
(48 streams of [1, 192, 32, 24]; tests/synth.make_latent - NOT real images' latents: no trained checkpoint exists offline).

  1. time: ``quantize_rdo_batch`` against ``estimate_bits_batch`` on the same inputs in the same run, HIP events on the launch's stream
     around each call, after warm-up.  Both calls are census kernels + ONE CDF kernel (rdoq_kernel / rate_kernel) + a few KB back; the
     RDOQ call runs the census twice (over y and over its result).  Per-kernel durations: run this script under
     ``rocprofv3 --kernel-trace --stats -- python scripts/rdoq_time.py --reps 20`` and read the kernel rows.
  2. rate and distortion for lambda in {0.02, 0.1, 0.5}: bytes of ``compress_batch`` with and without RDOQ (true stream lengths), the
     mean squared error RDOQ adds over plain rounding (torch, float64), latents moved.

Prints one JSON object; profiles/rdoq.md records a run."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--mode", default="polya")
    ap.add_argument("--no-rd", action="store_true", help="timing only (profiler runs)")
    a = ap.parse_args()
    import bench
    from flashgmm_amd import GaussianMixtureConditional

    dev = torch.device("cuda:0")
    _, devt, _ = bench.make_workload(0, a.images, dev, "kodak24", keep_host_images=0)
    y, s, m, w = (torch.cat([st[k] for st in devt]) for k in range(4))  # stacked [N, ...]
    gmc = GaussianMixtureConditional(K=4, mode=a.mode)
    n_lat = y.numel()
    out = {"workload": f"kodak24 synthetic, {a.images} images, {y.shape[0]} streams, {n_lat} latents", "mode": a.mode}
    est = timed(lambda: gmc.estimate_bits_batch(y, s, m, w), a.reps, a.warmup)
    rdo = timed(lambda: gmc.quantize_rdo_batch(y, s, m, w, 0.1), a.reps, a.warmup)
    out["estimate_call"], out["rdoq_call"] = est, rdo
    out["call_ratio"] = round(rdo["median_ms"] / est["median_ms"], 3)
    if not a.no_rd:
        base = gmc.compress_batch(y, s, m, w)
        base_bytes = sum(len(b) for (b, _, _), _ in base)
        yd = y.double()
        mse0 = float(((yd - torch.round(y).double()) ** 2).mean())
        out["plain"] = {"bytes": base_bytes, "mse": round(mse0, 6)}
        out["rd"] = []
        for lam in (0.02, 0.1, 0.5):
            q = gmc.quantize_rdo_batch(y, s, m, w, lam)
            yq = torch.cat([r.y for r in q])
            enc = gmc.compress_batch(yq, s, m, w)
            nb = sum(len(b) for (b, _, _), _ in enc)
            mse = float(((yd - yq.double()) ** 2).mean())
            out["rd"].append({"lambda": lam, "bytes": nb, "bytes_saved_frac": round(1 - nb / base_bytes, 4), "mse": round(mse, 6),
                              "mse_added": round(mse - mse0, 6), "moved_frac": round(sum(r.n_changed for r in q) / n_lat, 4),
                              "bits_q_saved_frac": round(1 - sum(r.bits_q_after for r in q) / sum(r.bits_q_before for r in q), 4)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
