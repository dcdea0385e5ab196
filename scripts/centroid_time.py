#!/usr/bin/env python3
"""Time the centroid call (include/flashgmm_amd.h section 3i, centroid_kernel) beside the likelihood call's forward with the map (section
3g, like_kernel) on a Kodak batch: 48 x y [192, 32, 24] with float32 and float16 planes.  Not a test and not bench.py's workload; the
protocol is scripts/likelihood_time.py's.

Both calls go through ctypes on item arrays and outputs built once, so a window holds the two native calls and nothing of Python's: one
upload of descriptors, one memset, ONE kernel, one small copy back and the call's wait each.  Device events around ``--reps`` calls
after ``--warmup`` calls, the median of ``--rounds`` such windows with [min .. max]; the two calls alternate window by window in one
process.  Both kernels read 52 B (28 B with two-byte planes) and write 4 B per latent.  Beside them: the header's binary32 sequence as torch
evaluates it on the GPU (tests/centroid_ref.py), the way profiles/likelihood.md times torch eager.  One JSON line at the end.  For the
kernels alone, run this under ``rocprofv3 --kernel-trace --stats``.

    python scripts/centroid_time.py [--items 48] [--reps 20] [--rounds 7] [--warmup 3]
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

from flashgmm_amd import _lib  # noqa: E402
from tests import centroid_ref as Z  # noqa: E402
from tests import like_ref as R  # noqa: E402

DEV = "cuda:0"


def inputs(B, M, h, w, dtype):
    rng = np.random.default_rng(7)
    n = (B, 4, M, h, w)
    sg = (np.exp(rng.uniform(-3, 2.5, (B, 1, M, h, w))) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    base = rng.standard_normal((B, M, h, w)) * 4
    mu = (base[:, None] + rng.standard_normal(n) * sg * 1.5).astype(np.float32)
    y = np.round(base + rng.standard_normal((B, M, h, w)) * sg.mean(1) * 1.5).astype(np.float32)  # a decoder's y_hat
    lg = rng.standard_normal(n)
    pi = (np.exp(lg) / np.exp(lg).sum(1, keepdims=True)).astype(np.float32)
    return [torch.from_numpy(y).to(DEV)] + [torch.from_numpy(a.reshape(B, 4 * M, h, w)).to(DEV).to(dtype) for a in (sg, mu, pi)]


def items_of(struct, y, s, m, w, **outs):
    B, M, h, wd = y.shape
    arr = (struct * B)()
    for i, it in enumerate(arr):
        it.y = y[i].data_ptr()
        it.params = _lib.fgmm_params(s[i].data_ptr(), m[i].data_ptr(), w[i].data_ptr(), M * h * wd, h * wd, {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[s.dtype], 0)
        it.M, it.K, it.hw = M, 4, h * wd
        for name, t in outs.items():
            setattr(it, name, t[i].data_ptr())
    return arr


def window(f, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


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
    L, ctx = _lib.lib(), _lib.ctx(0)
    res = {"items": B, "shape": [M, h, w], "latents": n}
    for dtype, name in ((torch.float32, "float32"), (torch.float16, "float16")):
        y, s, m, wt = inputs(B, M, h, w, dtype)
        rec, like = torch.empty_like(y), torch.empty_like(y)
        c_items = items_of(_lib.fgmm_centroid_item, y, s, m, wt, rec=rec)
        l_items = items_of(_lib.fgmm_like_item, y, s, m, wt, like_out=like)
        stream = torch.cuda.current_stream().cuda_stream

        def centroid():
            _lib.check(L.fgmm_gmc_centroid_batch(ctx, stream, c_items, B, R.SB, Z.P_MIN))

        def likelihood():
            _lib.check(L.fgmm_gmc_likelihood_batch(ctx, stream, l_items, B, 1, R.SB, R.LB))

        wide = [t.to(torch.float32) for t in (s, m, wt)]

        def restated():
            return Z.centroid(y, *wide)["rec"]

        for f in (centroid, likelihood, restated):
            for _ in range(args.warmup):
                f()
        torch.cuda.synchronize()
        tc, tl, tt = [], [], []
        for _ in range(args.rounds):  # alternating: the host is shared
            tc.append(window(centroid, args.reps))
            tl.append(window(likelihood, args.reps))
        for _ in range(3):
            tt.append(window(restated, 3))
        kept = sum(int(it.n_kept) for it in c_items)
        diff = float((rec - restated()).abs().max())
        r = {"centroid_ms": statistics.median(tc), "centroid_ms_min_max": [min(tc), max(tc)], "likelihood_ms": statistics.median(tl),
             "likelihood_ms_min_max": [min(tl), max(tl)], "ratio": statistics.median(tc) / statistics.median(tl), "torch_restatement_ms": statistics.median(tt),
             "kept_share": kept / n, "max_abs_diff_to_restatement": diff}
        print(f"  {name:8s} planes, {n} latents: centroid call {r['centroid_ms']:.3f} ms [{min(tc):.3f} .. {max(tc):.3f}]   likelihood call (map) "
              f"{r['likelihood_ms']:.3f} ms [{min(tl):.3f} .. {max(tl):.3f}]   ratio {r['ratio']:.3f}   torch restatement {r['torch_restatement_ms']:.2f} ms   "
              f"kept {100 * r['kept_share']:.1f} %   largest |kernel - restatement| {diff:.2e}")
        res[name] = r
    print(json.dumps(res))


if __name__ == "__main__":
    main()
