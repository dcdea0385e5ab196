"""The parameter network's hidden layers, measured (profiles/param_body.md): ParameterBody.features (fgmm_hidden.hip: one launch per
layer, the merge folded into the first layer's K loop, the activation into the epilogue) against the path it replaces - torch.cat,
conv2d, leaky_relu, conv2d, leaky_relu with torch's convolution (MIOpen, warmed) - at the reference model's widths, c_ctx = c_side = 384
-> 640 -> 640 with LeakyReLU, on a Kodak half (hw = 768 positions: 32 x 24), for N = 24 and N = 1.

GPU time by device events on the current stream: a sample is `inner` back-to-back calls between two events, divided by `inner`; the two
paths (and each layer of the new one alone, and the anchors' form: an absent context against a zeros tensor) alternate sample by sample
in one process; the median and the minimum of `samples` samples after `warm` warm-up samples of each.  The share of the f32 MFMA roof
(157.3 TF, as profiles/r06_head_kernel.md) counts the multiply-adds the definition needs, 2 * c_out * c_in per position.  The block
height is the header's rule (section 2c) evaluated for this device.  Needs a GPU: fails without one.
With a fourth argument `bf16x6` the bf16x6 form (fgmm_hidden16.hip; profiles/param_body_bf16x6.md) joins the alternation: the whole call -
both splits, the bf16x6 kernel and the flagged-items launch of every layer - and each layer alone, against the f32 form and torch in the
same process; its share of the BF16 roof (419.5 TF of six part products per product, as profiles/ckbd_context_bf16x6.md).
usage: python scripts/param_body_bench.py [samples=30] [inner=10] [warm=5] [bf16x6]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from flashgmm_amd import ParameterBody  # noqa: E402

samples = int(sys.argv[1]) if len(sys.argv) > 1 else 30
inner = int(sys.argv[2]) if len(sys.argv) > 2 else 10
warm = int(sys.argv[3]) if len(sys.argv) > 3 else 5
B16 = len(sys.argv) > 4 and sys.argv[4] == "bf16x6"
ROOF16_TF = 419.5
C_CTX, C_SIDE, C_HID, h, w = 384, 384, 640, 32, 24
ROOF_TF = 157.3
assert torch.cuda.is_available(), "scripts/param_body_bench.py needs a GPU"
dev = "cuda:0"
CUS = torch.cuda.get_device_properties(0).multi_processor_count

torch.manual_seed(1)
body = torch.nn.Sequential(torch.nn.Conv2d(C_CTX + C_SIDE, C_HID, 1), torch.nn.LeakyReLU(), torch.nn.Conv2d(C_HID, C_HID, 1), torch.nn.LeakyReLU()).to(dev)
op = ParameterBody(body, C_CTX)
layer1, layer2 = ParameterBody(body[:2], C_CTX), ParameterBody(body[2:], 0)
if B16:
    op16, layer1_16, layer2_16 = (ParameterBody(m, c, arithmetic="bf16x6") for m, c in ((body, C_CTX), (body[:2], C_CTX), (body[2:], 0)))


def height(n, hw, c_out):
    outer, n_rt = n * -(-hw // 128), -(-c_out // 32)
    return next((T for T in (5, 2) if outer * -(-n_rt // T) >= CUS), 1)


def sample(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, r


out = {"workload": f"hidden layers {C_CTX} + {C_SIDE} -> {C_HID} -> {C_HID}, LeakyReLU, {h} x {w} = {h * w} positions per item", "compute_units": CUS,
       "samples": samples, "calls_per_sample": inner, "warmup_samples": warm, "roof_tf": ROOF_TF}
for N in (24, 1):
    ctx, side = torch.randn((N, C_CTX, h, w), device=dev), torch.randn((N, C_SIDE, h, w), device=dev)
    mid = layer1.features(ctx, side)

    def torch_path(c=ctx):
        with torch.no_grad():
            return body(torch.cat((c, side), 1))

    paths = {"kernel": lambda: op.features(ctx, side), "torch": torch_path, "kernel_layer1": lambda: layer1.features(ctx, side),
             "kernel_layer2": lambda: layer2.features(None, mid), "kernel_anchors": lambda: op.features(None, side),
             "torch_anchors": lambda: torch_path(torch.zeros_like(ctx))}
    if B16:
        paths.update({"bf16x6": lambda: op16.features(ctx, side), "bf16x6_layer1": lambda: layer1_16.features(ctx, side),
                      "bf16x6_layer2": lambda: layer2_16.features(None, mid), "bf16x6_anchors": lambda: op16.features(None, side)})
    for _ in range(warm):
        for fn in paths.values():
            sample(fn)
    t = {k: [] for k in paths}
    for _ in range(samples):
        for k, fn in paths.items():
            t[k].append(sample(fn)[0])
    res = {k: {"median_ms": round(float(np.median(v)), 5), "min_ms": round(float(np.min(v)), 5)} for k, v in t.items()}
    for k, c_in in (("kernel_layer1", C_CTX + C_SIDE), ("kernel_layer2", C_HID)):
        flop = 2.0 * C_HID * c_in * N * h * w
        res[k]["tflops"] = round(flop / res[k]["median_ms"] / 1e9, 2)
        res[k]["frac_of_roof"] = round(flop / res[k]["median_ms"] / 1e9 / ROOF_TF, 4)
    res["block_height"] = height(N, h * w, C_HID)
    res["blocks"] = N * -(-h * w // 128) * -(-(C_HID // 32) // res["block_height"])
    if B16:
        for k, c_in in (("bf16x6_layer1", C_CTX + C_SIDE), ("bf16x6_layer2", C_HID)):
            flop = 2.0 * C_HID * c_in * N * h * w
            res[k]["tflops"] = round(flop / res[k]["median_ms"] / 1e9, 2)
            res[k]["frac_of_bf16_roof"] = round(flop / res[k]["median_ms"] / 1e9 / ROOF16_TF, 4)
        res["bf16x6_over_kernel"] = round(res["bf16x6"]["median_ms"] / res["kernel"]["median_ms"], 4)
        res["kernel_over_bf16x6"] = round(res["kernel"]["median_ms"] / res["bf16x6"]["median_ms"], 4)
        res["bf16x6_over_torch"] = round(res["bf16x6"]["median_ms"] / res["torch"]["median_ms"], 4)
        res["anchors_bf16x6_over_kernel"] = round(res["bf16x6_anchors"]["median_ms"] / res["kernel_anchors"]["median_ms"], 4)
        res["max_abs_diff_bf16x6_to_kernel"] = float((op16.features(ctx, side) - op.features(ctx, side)).abs().max())
    res["kernel_over_torch"] = round(res["kernel"]["median_ms"] / res["torch"]["median_ms"], 4)
    res["anchors_kernel_over_torch"] = round(res["kernel_anchors"]["median_ms"] / res["torch_anchors"]["median_ms"], 4)
    res["max_abs_diff_to_torch"] = float((torch_path() - op.features(ctx, side)).abs().max())
    out[f"N={N}"] = res
print(json.dumps(out))
