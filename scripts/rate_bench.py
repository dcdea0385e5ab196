#!/usr/bin/env python3
"""The size estimate against the coder it predicts, on bench.py's Kodak batch: 48 halves [1, 192, 32, 24], float32 planes, resident
in HBM (bench.make_workload: the same seeds, the same arrays).

    timeout 300 python scripts/rate_bench.py [--reps 20] [--warmup 5] [--out FILE]
    timeout 600 rocprofv3 --kernel-trace --stats -d DIR -- python scripts/rate_bench.py     # rate_kernel against symtab_kernel

Prints one JSON line: the median wall time of ``estimate_bits_batch`` and of ``compress_batch`` (what a caller has to run today to
learn the size) on the stacked batch, per Phi approximation; and how often the predicted length IS the length of compress_batch's
bitstream, over the 48 x 3 streams.  Both calls run in this process on the same tensors, so one kernel trace holds rate_kernel's and
symtab_kernel's times side by side (profiles/rate_estimate.md).  Numbers go to profiles/, never into code or assertions."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import bench
    from flashgmm_amd import GaussianMixtureConditional

    dev = torch.device("cuda:0")
    _, devt, _ = bench.make_workload(0, a.images, dev, "kodak24", False, keep_host_images=0)
    y, sg, mu, pi = (torch.cat([st[k] for st in devt]) for k in range(4))  # [48, ...]: the stacked form
    torch.cuda.synchronize()

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return ts

    res = {"streams": int(y.shape[0]), "shape": list(y.shape[1:]), "reps": a.reps, "warmup": a.warmup, "modes": {}}
    equal = total = 0
    for mode in ("polya", "as", "logistic"):
        gmc = GaussianMixtureConditional(K=4, mode=mode)
        est = gmc.estimate_bits_batch(y, sg, mu, pi)
        enc = gmc.compress_batch(y, sg, mu, pi)
        lens = [len(b) for b in enc.strings]
        hit = sum(e.nbytes == n for e, n in zip(est, lens))
        off = sorted({e.nbytes - n for e, n in zip(est, lens)})
        assert [e.abs_max for e in est] == list(enc.abs_maxes) and all(e.zero_bitmap.tolist() == z.tolist() for e, z in zip(est, enc.zero_bitmaps))
        equal, total = equal + hit, total + len(lens)
        t_est = timed(lambda: gmc.estimate_bits_batch(y, sg, mu, pi))
        t_map = timed(lambda: gmc.estimate_bits_batch(y, sg, mu, pi, per_channel=True, per_latent=True))
        t_enc = timed(lambda: gmc.compress_batch(y, sg, mu, pi))
        res["modes"][mode] = {"estimate_ms_median": round(statistics.median(t_est), 4), "estimate_ms_min": round(min(t_est), 4),
                              "estimate_with_maps_ms_median": round(statistics.median(t_map), 4),
                              "compress_ms_median": round(statistics.median(t_enc), 4), "compress_ms_min": round(min(t_enc), 4),
                              "ratio": round(statistics.median(t_est) / statistics.median(t_enc), 4),
                              "nbytes_equal": hit, "nbytes_differences": off, "bytes_total": sum(lens),
                              "bits_total": round(sum(e.bits for e in est), 3), "n_bypass": sum(e.n_bypass for e in est)}
    res["nbytes_equal"], res["nbytes_streams"] = equal, total
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
