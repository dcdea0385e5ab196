"""The checkerboard context convolution, measured (profiles/ckbd_context.md): CheckerboardContext.non_anchor (fgmm_ckbd_ctx.hip: the 12
kept taps at the non-anchor positions, one launch) against the path it replaces, unembed(conv(embed([anchors, 0])))[1] with torch's
convolution (MIOpen, warmed) between the library's own embed and unembed kernels - at the Kodak latent, M = 192, C_out = 384, h = 32,
w = 48 (768 compact positions per image), for N = 1 and N = 24 images.

GPU time by device events on the current stream: a sample is `inner` back-to-back calls between two events, divided by `inner` (one
call of N = 1 is tens of microseconds: near the resolution of an event pair); the two paths alternate sample by sample in one process;
the median and the minimum of `samples` samples after `warm` warm-up samples of each.  The fraction of the f32 MFMA roof (157.3 TF, as
profiles/r06_head_kernel.md) counts the multiply-adds the definition needs, 2 * C_out * 12 M per compact position.
usage: python scripts/ckbd_context_bench.py [samples=30] [inner=10] [warm=5]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flashgmm_amd.ops import CheckerboardContext, ckbd_embed, ckbd_unembed  # noqa: E402

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 30
inner = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
M, C_out, h, w = 192, 384, 32, 48
ROOF_TF = 157.3
dev = "cuda:0"

torch.manual_seed(1)
conv = torch.nn.Conv2d(M, C_out, 5, padding=2).to(dev)
mask = torch.zeros((C_out, M, 5, 5), device=dev)
mask.view(C_out, M, 25)[:, :, 1::2] = 1  # the kernel positions (i, j) with i + j odd
with torch.no_grad():
    conv.weight.mul_(mask)
op = CheckerboardContext(conv, "even")


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, r


out = {"workload": f"context conv {M} -> {C_out}, 5x5 checkerboard-masked, latent {h} x {w} ({h * w // 2} compact positions per image)",
       "samples": samples, "calls_per_sample": inner, "warmup_samples": warm, "roof_tf": ROOF_TF}
for N in (1, 24):
    anchors = torch.round(torch.randn((N, M, h, w // 2), device=dev) * 4)
    zeros = torch.zeros_like(anchors)

    def torch_path():
        with torch.no_grad():
            return ckbd_unembed(conv(ckbd_embed(torch.stack([anchors, zeros]), "even")), "even")[1]

    def conv_only(full=ckbd_embed(torch.stack([anchors, zeros]), "even")):
        with torch.no_grad():
            return conv(full)

    paths = {"kernel": lambda: op.non_anchor(anchors), "torch": torch_path, "torch_conv_alone": conv_only}
    for _ in range(warm):
        for fn in paths.values():
            sample(fn)
    t = {k: [] for k in paths}
    for _ in range(samples):
        for k, fn in paths.items():
            t[k].append(sample(fn)[0])
    ref, got = torch_path(), op.non_anchor(anchors)
    flop = 2.0 * C_out * 12 * M * N * h * (w // 2)
    res = {k: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(np.min(v)), 5)} for k, v in t.items()}
    km = res["kernel"]["median_ms"]
    res["kernel"]["tflops"] = round(flop / km / 1e9, 2)
    res["kernel"]["frac_of_roof"] = round(flop / km / 1e9 / ROOF_TF, 4)
    res["gflop_needed"] = round(flop / 1e9, 3)
    res["kernel_over_torch"] = round(km / res["torch"]["median_ms"], 4)
    res["max_abs_diff_to_torch"] = float((ref - got).abs().max())
    out[f"N={N}"] = res
print(json.dumps(out))
