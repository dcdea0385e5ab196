"""The checkerboard context convolution under autograd, measured (profiles/ckbd_context_grad.md): forward + backward of
flashgmm_amd.ops.checkerboard_context (fgmm_ckbd_ctx.hip forward and data gradient, fgmm_ckbd_ctx_grad.hip weight and bias gradients)
against the torch path for the same thing - ckbd_embed, conv2d with the masked weight (MIOpen, warmed), ckbd_unembed, under autograd -
with M = 192, C_out = 384 at the training shape N = 8, h = w = 16 and at N = 24, h = 32, w = 48.  Both paths differentiate with respect
to the anchors, the weight (through weight * mask) and the bias.

The protocol of scripts/ckbd_context_bench.py: GPU time by device events on the current stream, a sample is `inner` back-to-back
forward + backward passes between two events, divided by `inner`; the paths alternate sample by sample in one process; the median and
the minimum of `samples` samples after `warm` warm-up samples of each.  `wgrad` alone is fgmm_ckbd_ctx_wgrad through the C ABI (both
outputs, the workspace allocated once); its TF count the multiply-adds the definition needs, 2 * C_out * 12 M per compact position,
against the 157.3 TF roof of profiles/ckbd_context.md.
usage: python scripts/ckbd_context_grad_bench.py [samples=30] [inner=5] [warm=5]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flashgmm_amd import _lib  # noqa: E402
from flashgmm_amd.ops import checkerboard_context, ckbd_embed, ckbd_unembed  # noqa: E402

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 30
inner = int(sys.argv[2]) if len(sys.argv) > 2 else 5
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
M, C_out = 192, 384
ROOF_TF = 157.3
dev = "cuda:0"

torch.manual_seed(1)
weight = (torch.randn((C_out, M, 5, 5), device=dev) / (12 * M) ** 0.5).requires_grad_(True)
bias = torch.randn((C_out,), device=dev).requires_grad_(True)
mask = torch.zeros((C_out, M, 5, 5), device=dev)
mask.view(C_out, M, 25)[:, :, 1::2] = 1  # the kernel positions (i, j) with i + j odd


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, r


out = {"workload": f"context conv {M} -> {C_out}, 5x5 checkerboard-masked, forward + backward (anchors, weight, bias)",
       "samples": samples, "passes_per_sample": inner, "warmup_samples": warm, "roof_tf": ROOF_TF}
for N, h, w in ((8, 16, 16), (24, 32, 48)):
    anchors = (torch.round(torch.randn((N, M, h, w // 2), device=dev) * 4) + torch.rand((N, M, h, w // 2), device=dev) - 0.5).requires_grad_(True)
    zeros = torch.zeros_like(anchors)
    g = torch.randn((N, C_out, h, w // 2), device=dev)

    def grads(y):
        return torch.autograd.grad(y, (anchors, weight, bias), g)

    def kernel_path():
        return grads(checkerboard_context(anchors, weight * mask, bias, "even"))

    def torch_path():
        full = ckbd_embed(torch.stack([anchors, zeros]), "even")
        return grads(ckbd_unembed(torch.nn.functional.conv2d(full, weight * mask, bias, padding=2), "even")[1])

    L, ctx = _lib.lib(), _lib.ctx(0)
    nbytes = L.fgmm_ckbd_ctx_wgrad_workspace(M, C_out, N, h, w)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    dw, db = torch.empty_like(weight), torch.empty_like(bias)
    a_ = anchors.detach()

    def wgrad_alone():
        _lib.check(L.fgmm_ckbd_ctx_wgrad(ctx, torch.cuda.current_stream().cuda_stream, a_.data_ptr(), g.data_ptr(), M, C_out, N, h, w, 0,
                                         dw.data_ptr(), db.data_ptr(), ws.data_ptr(), nbytes), "wgrad")

    paths = {"kernel": kernel_path, "torch": torch_path, "wgrad_alone": wgrad_alone}
    for _ in range(warm):
        for fn in paths.values():
            sample(fn)
    t = {k: [] for k in paths}
    for _ in range(samples):
        for k, fn in paths.items():
            t[k].append(sample(fn)[0])
    ref, got = torch_path(), kernel_path()
    flop = 2.0 * C_out * 12 * M * N * h * (w // 2)
    res = {k: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(np.min(v)), 5)} for k, v in t.items()}
    wm = res["wgrad_alone"]["median_ms"]
    res["wgrad_alone"]["tflops"] = round(flop / wm / 1e9, 2)
    res["wgrad_alone"]["frac_of_roof"] = round(flop / wm / 1e9 / ROOF_TF, 4)
    res["gflop_needed_per_gradient"] = round(flop / 1e9, 3)
    res["workspace_mb"] = round(nbytes / 1e6, 2)
    res["kernel_over_torch"] = round(res["kernel"]["median_ms"] / res["torch"]["median_ms"], 4)
    res["max_abs_diff_to_torch"] = {n: float((r - k).abs().max()) for n, r, k in zip(("anchors", "weight", "bias"), ref, got)}
    out[f"N={N},h={h},w={w}"] = res
print(json.dumps(out))
