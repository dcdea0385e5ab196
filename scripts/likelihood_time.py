#!/usr/bin/env python3
"""Time the entropy model's forward() (include/flashgmm_amd.h section 3g) against torch eager on a Kodak batch: 48 items of
[192, 32, 24] with float32 planes, then the same with float16 planes.  Not a test and not bench.py's workload.

Three calls - forward with the likelihood map, ``rate_bits`` alone, forward plus backward - each as the fused kernels run it and as
torch eager evaluates tests/like_ref.py's float32 formula with autograd on the same tensors (``autograd_forward``: the reference's own
sequence of operations).  Device events around ``--reps`` calls after ``--warmup`` calls, the median of ``--rounds`` such windows; the
two sides alternate window by window.  ``torch.cuda.max_memory_allocated`` over one forward plus backward, for both.  The call times
include what the call does besides its kernel (descriptors, the wait for the sums); the algorithmic bytes at 8 TB/s are printed beside
them.  One JSON line per plane type at the end.

    python scripts/likelihood_time.py [--items 48] [--reps 20] [--rounds 7] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flashgmm_amd import GaussianMixtureConditional  # noqa: E402
from tests import like_ref as R  # noqa: E402

DEV = "cuda:0"
HBM = 8.0e12  # bytes per second, MI355X


def inputs(B, M, h, w, dtype):
    rng = np.random.default_rng(7)
    n = (B, 4, M, h, w)
    sg = (np.exp(rng.uniform(-3, 2.5, (B, 1, M, h, w))) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    base = rng.standard_normal((B, M, h, w)) * 4
    mu = (base[:, None] + rng.standard_normal(n) * sg * 1.5).astype(np.float32)
    y = (base + rng.standard_normal((B, M, h, w)) * sg.mean(1) * 1.5).astype(np.float32)
    lg = rng.standard_normal(n)
    pi = (np.exp(lg) / np.exp(lg).sum(1, keepdims=True)).astype(np.float32)
    t = [torch.from_numpy(y).to(DEV)] + [torch.from_numpy(a.reshape(B, 4 * M, h, w)).to(DEV).to(dtype) for a in (sg, mu, pi)]
    g = torch.from_numpy(rng.standard_normal((B, M, h, w)).astype(np.float32)).to(DEV)
    return t, g


def window(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, fused, eager, args):
    for f in (fused, eager):
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    tf, te = [], []
    for _ in range(args.rounds):  # alternating: the host is shared
        tf.append(window(fused, args.reps))
        te.append(window(eager, args.reps))
    r = {"fused_ms": statistics.median(tf), "eager_ms": statistics.median(te), "fused_ms_min_max": [min(tf), max(tf)], "eager_ms_min_max": [min(te), max(te)]}
    print(f"  {name:22s} fused {r['fused_ms']:8.3f} ms [{min(tf):.3f} .. {max(tf):.3f}]   eager {r['eager_ms']:8.3f} ms [{min(te):.3f} .. {max(te):.3f}]   "
          f"x{r['eager_ms'] / r['fused_ms']:.2f}")
    return r


def peak(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=48)
    ap.add_argument("--shape", type=int, nargs=3, default=[192, 32, 24])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    B, (M, h, w) = args.items, args.shape
    n = B * M * h * w
    gmc = GaussianMixtureConditional(K=4).eval()
    for dtype in (torch.float32, torch.float16):
        (y, s, m, wt), g = inputs(B, M, h, w, dtype)
        pb = 4 if dtype == torch.float32 else 2
        algo = {"forward_map": n * (4 + 12 * pb + 4), "rate_bits": n * (4 + 12 * pb), "forward_backward": n * (4 + 12 * pb + 4) + n * (8 + 12 * pb + 52)}
        print(f"{B} x [{M}, {h}, {w}], {dtype} planes: {n} latents")
        leaves = lambda: [t.detach().requires_grad_(True) for t in (y, s, m, wt)]  # noqa: E731

        def fused_fb():
            lv = leaves()
            gmc.likelihood(*lv)[1].backward(g)

        def eager_fb():
            lv = leaves()
            R.autograd_forward(*lv).backward(g)

        def eager_fwd():
            with torch.no_grad():
                R.autograd_forward(y, s, m, wt)

        def eager_rate():
            with torch.no_grad():
                (-torch.log2(R.autograd_forward(torch.round(y), s, m, wt).double())).sum((1, 2, 3))

        with torch.no_grad():
            same = torch.equal(gmc.likelihood(y, s, m, wt)[1], R.autograd_forward(y, s.float(), m.float(), wt.float()))
        print(f"  fused likelihood == eager float32 likelihood (on widened planes), bit for bit: {same}")
        res = {"planes": str(dtype), "items": B, "shape": [M, h, w], "latents": n, "bit_identical_to_eager": same}
        for name, fused, eager in (("forward_map", lambda: gmc.likelihood(y, s, m, wt), eager_fwd), ("rate_bits", lambda: gmc.rate_bits(y, s, m, wt), eager_rate),
                                   ("forward_backward", fused_fb, eager_fb)):
            r = compare(name, fused, eager, args)
            r["algorithmic_bytes"] = algo[name]
            r["algorithmic_ms_at_8TBps"] = 1e3 * algo[name] / HBM
            print(f"  {'':22s} algorithmic {algo[name] / 1e6:.1f} MB = {r['algorithmic_ms_at_8TBps']:.4f} ms at 8 TB/s: fused call at "
                  f"{100 * r['algorithmic_ms_at_8TBps'] / r['fused_ms']:.1f} % of it")
            res[name] = r
        res["peak_bytes_forward_backward"] = {"fused": peak(fused_fb), "eager": peak(eager_fb)}
        print(f"  peak memory over one forward + backward: fused {res['peak_bytes_forward_backward']['fused'] / 2**20:.1f} MiB, "
              f"eager {res['peak_bytes_forward_backward']['eager'] / 2**20:.1f} MiB")
        print(json.dumps(res))


if __name__ == "__main__":
    main()
