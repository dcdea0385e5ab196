#!/usr/bin/env python3
"""Time the fused entropy-bottleneck forward + backward (include/flashgmm_amd.h section 3j, ``flashgmm_amd.EntropyBottleneck``) against the
torch float32 restatement of the same arithmetic (tests/eb_ref.py: eager torch, autograd's backward), in one process, on the shapes the
hyper-latent has in practice.  Per shape: 10 warm-up steps, then the median of 50; a step is the likelihood of a batch in training mode
(noise drawn outside the timed region), the loss ``sum(-log2 likelihood)`` and its backward into x and every parameter.  Prints one JSON
line per shape; the figures go into profiles/entropy_bottleneck.md."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from flashgmm_amd import EntropyBottleneck  # noqa: E402
from tests import eb_ref as R  # noqa: E402

SHAPES = {"training crop": (16, 192, 4, 4), "Kodak batch": (24, 192, 8, 12), "one 4K image": (1, 192, 34, 60)}
WARMUP, STEPS = 10, 50


def timed(step):
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(STEPS):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms)


def main():
    dev = "cuda:0"
    for name, shape in SHAPES.items():
        torch.manual_seed(1)
        eb = EntropyBottleneck(shape[1]).to(dev).train()
        with torch.no_grad():
            for n in R.NAMES:  # away from the initial values: factors that are not zero
                if "factor" in n:
                    getattr(eb, n).normal_(0, 0.5)
        x = (torch.randn(shape, device=dev) * 6).requires_grad_(True)
        noised = (x + torch.empty_like(x).uniform_(-0.5, 0.5)).detach().requires_grad_(True)
        params = {n: getattr(eb, n) for n in R.NAMES}
        med = eb._get_medians().reshape(-1)

        def fused():
            eb.zero_grad(set_to_none=True)
            noised.grad = None
            _, like = eb.likelihood(noised)
            like.log2().sum().neg().backward()

        def eager():
            eb.zero_grad(set_to_none=True)
            noised.grad = None
            like = R.forward(noised, params, med, 0, sig=torch.sigmoid)["out"]
            like.log2().sum().neg().backward()

        def fused_rate():
            eb.zero_grad(set_to_none=True)
            noised.grad = None
            _, bits = eb.rate_bits(noised, training=False)  # (evaluation mode: no noise is drawn inside the timed region)
            bits.sum().backward()

        out = {"shape": list(shape), "name": name, "fused_ms": round(timed(fused), 4), "eager_ms": round(timed(eager), 4),
               "fused_rate_bits_eval_ms": round(timed(fused_rate), 4)}
        out["speedup"] = round(out["eager_ms"] / out["fused_ms"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
