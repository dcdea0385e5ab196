#!/usr/bin/env python3
"""Time a training step's rate term from the parameter head's output, with the softmax over K in torch (path A) and in the likelihood
kernels (path B, include/flashgmm_amd.h section 3h), on a Kodak batch: the head's output [48, 2304, 32, 24] float32 with y
[48, 192, 32, 24].  Not a test and not bench.py's workload; the protocol is scripts/likelihood_time.py's.

  A  ``chunk(3, 1)`` -> ``torch.softmax`` on the [B, 4, M, h, w] view -> ``GaussianMixtureConditional.forward`` / ``rate_bits`` (section
     3g) -> ``.backward()``: torch's softmax backward, then the concatenation in the backward of ``chunk``
  B  ``forward_params`` / ``rate_bits_params`` -> ``.backward()``: one kernel each way, the gradient of the head's output written once

Two steps, both in training mode (the same uniform noise is drawn by torch in either path) so that ``y`` receives a gradient: forward
with the likelihood map plus backward at a fixed upstream gradient, and ``rate_bits`` plus backward of the summed bits.  Device events
around ``--reps`` steps after ``--warmup`` steps, the median of ``--rounds`` such windows with [min .. max]; the two paths alternate
window by window in one process.  The yardstick is A: B's median against A's fastest window.  ``torch.cuda.max_memory_allocated`` over
one step above what the inputs hold, for both.  One JSON line at the end.

    python scripts/likelihood_logits_time.py [--items 48] [--reps 20] [--rounds 7] [--warmup 3]
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

DEV = "cuda:0"
# bytes per latent around the two kernels in path A, K = 4, float32: the softmax reads and writes [K] (32); its backward reads the kept
# weights and dweights and writes the logits' gradient (48); the backward of chunk reads three [K] gradients and writes them again (96)
TORCH_BYTES = {"softmax forward": 32, "softmax backward": 48, "concatenation in the backward of chunk": 96}
KERNEL_BYTES = {"like_kernel": 56, "like_bwd_kernel": 108}


def inputs(B, M, h, w):
    rng = np.random.default_rng(7)
    n = (B, 4, M, h, w)
    sg = (np.exp(rng.uniform(-3, 2.5, (B, 1, M, h, w))) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    base = rng.standard_normal((B, M, h, w)) * 4
    mu = (base[:, None] + rng.standard_normal(n) * sg * 1.5).astype(np.float32)
    y = (base + rng.standard_normal((B, M, h, w)) * sg.mean(1) * 1.5).astype(np.float32)
    lg = (2.0 * rng.standard_normal(n)).astype(np.float32)
    params = torch.cat([torch.from_numpy(a.reshape(B, 4 * M, h, w)).to(DEV) for a in (sg, mu, lg)], 1)
    g = torch.from_numpy(rng.standard_normal((B, M, h, w)).astype(np.float32)).to(DEV)
    return torch.from_numpy(y).to(DEV), params, g


def window(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def compare(name, path_a, path_b, args):
    for f in (path_a, path_b):
        for _ in range(args.warmup):
            f()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(args.rounds):  # alternating: the host is shared
        ta.append(window(path_a, args.reps))
        tb.append(window(path_b, args.reps))
    r = {"a_ms": statistics.median(ta), "b_ms": statistics.median(tb), "a_ms_min_max": [min(ta), max(ta)], "b_ms_min_max": [min(tb), max(tb)]}
    r["b_median_below_a_minimum"] = r["b_ms"] < min(ta)
    print(f"  {name:18s} A {r['a_ms']:8.3f} ms [{min(ta):.3f} .. {max(ta):.3f}]   B {r['b_ms']:8.3f} ms [{min(tb):.3f} .. {max(tb):.3f}]   "
          f"A - B {r['a_ms'] - r['b_ms']:.3f} ms   B's median below A's fastest window: {r['b_median_below_a_minimum']}")
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
    gmc = GaussianMixtureConditional(K=4).train()
    y, params, g = inputs(B, M, h, w)
    print(f"head output [{B}, {12 * M}, {h}, {w}] float32, y [{B}, {M}, {h}, {w}]: {n} latents")
    leaves = lambda: (y.detach().requires_grad_(True), params.detach().requires_grad_(True))  # noqa: E731

    def softmaxed(p):
        s, m, lg = p.chunk(3, 1)
        return s, m, torch.softmax(lg.reshape(B, 4, M, h, w), dim=1).reshape(B, 4 * M, h, w)

    def a_map():
        yl, pl = leaves()
        gmc(yl, *softmaxed(pl))[1].backward(g)
        return yl, pl

    def b_map():
        yl, pl = leaves()
        gmc.forward_params(yl, pl)[1].backward(g)
        return yl, pl

    def a_rate():
        yl, pl = leaves()
        gmc.rate_bits(yl, *softmaxed(pl))[1].sum().backward()
        return yl, pl

    def b_rate():
        yl, pl = leaves()
        gmc.rate_bits_params(yl, pl)[1].sum().backward()
        return yl, pl

    # the two paths price the same thing: the same noise, weights 2e-7 apart
    torch.manual_seed(3)
    ya, pa = a_map()
    torch.manual_seed(3)
    yb, pb = b_map()
    dp, dy = float((pa.grad - pb.grad).abs().max()), float((ya.grad - yb.grad).abs().max())
    print(f"  largest |A - B| in params.grad {dp:.3e} (largest |A| {float(pa.grad.abs().max()):.3e}), in y.grad {dy:.3e}; both gradients contiguous: "
          f"{pa.grad.is_contiguous() and pb.grad.is_contiguous()}")
    del ya, pa, yb, pb
    res = {"items": B, "shape": [M, h, w], "latents": n, "max_abs_diff_params_grad": dp, "max_abs_diff_y_grad": dy}
    for name, fa, fb in (("map + backward", a_map, b_map), ("rate + backward", a_rate, b_rate)):
        r = compare(name, fa, fb, args)
        r["peak_bytes"] = {"a": peak(fa), "b": peak(fb)}
        print(f"  {'':18s} peak memory over one step above the inputs: A {r['peak_bytes']['a'] / 2**20:.1f} MiB, B {r['peak_bytes']['b'] / 2**20:.1f} MiB")
        res[name.replace(" + ", "_")] = r
    torch_bytes, kernel_bytes = sum(TORCH_BYTES.values()), sum(KERNEL_BYTES.values())
    print(f"  counted bytes per latent: torch around the kernels {torch_bytes} ({', '.join(f'{k} {v}' for k, v in TORCH_BYTES.items())}), the two kernels "
          f"{kernel_bytes}; {torch_bytes * n / 1e6:.1f} MB per step = {1e3 * torch_bytes * n / 8.0e12:.4f} ms at 8 TB/s")
    res["counted_bytes_per_latent"] = {"torch": TORCH_BYTES, "kernels": KERNEL_BYTES}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
