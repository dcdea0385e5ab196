#!/usr/bin/env python3
"""Generate tests/golden/g11_entropy_bottleneck.npz from the REAL reference: its own ``EntropyBottleneck`` imported in place (as
make_golden_likelihood.py does for G10), run on the CPU on the corpus of tests/eb_ref.py with the corpus' parameters loaded into it -
in float64 (the module ``.double()``) with autograd through its own ``_likelihood`` and ``LowerBound``, and once in float32 for the
written form ``sigmoid(upper) - sigmoid(lower)``.  Runs only where the reference is present; what is committed is data plus this script.

The fixture (x, g, region [2, 6, 16, 16]; parameters under their state-dict names):
    x, g, region, med, p.<name>     the inputs, float32 (region int8: 0 body, 1 left tail, 2 right tail)
    L64, like64                     mode 0 (the values as they are): ``_likelihood`` before the bound and after it, float64
    like64_eval, v64_eval           ``forward(x, training=False)``: mode 1, the bounded likelihood and the dequantized outputs
    dx64, d64.<name>                autograd's float64 gradients of sum(like64 * g): x and the 14 parameters
    dmed64, d64_eval.<name>         the same of sum(like64_eval * g): the medians (``quantiles[:, 0, 1]``) and the 14 parameters
    L32_written                     mode 0 in float32, the reference's written form, before the bound
    sd.<key>                        the float32 module's state dict after ``update()`` (its tables included)
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from tests import eb_ref as R  # noqa: E402


def main():
    import torch

    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    mg.import_reference_entropy_models(O.ref_ans(""))
    from compressai.entropy_models.entropy_models import EntropyBottleneck

    x, p, med, g, region = R.corpus()
    out = dict(x=x, g=g, region=region, med=med, **{"p." + n: p[n] for n in R.NAMES})

    def module(dtype):
        eb = EntropyBottleneck(R.C)
        with torch.no_grad():
            for n in R.NAMES:
                getattr(eb, n).copy_(torch.from_numpy(p[n]))
            eb.quantiles[:, 0, 1] = torch.from_numpy(med)
        return eb.to(dtype).eval()

    def as_cn(t):  # [B, C, h, w] -> [C, 1, B*h*w], the layout of the class's _likelihood
        return t.permute(1, 0, 2, 3).reshape(R.C, 1, -1)

    def back(t):
        return t.reshape(R.C, x.shape[0], *x.shape[2:]).permute(1, 0, 2, 3)

    eb = module(torch.float64)
    gt = torch.from_numpy(g).double()
    xl = torch.from_numpy(x).double().requires_grad_(True)
    L, _, _ = eb._likelihood(as_cn(xl))
    like = eb.likelihood_lower_bound(L)
    out["L64"], out["like64"] = back(L.detach()).numpy(), back(like.detach()).numpy()
    (back(like) * gt).sum().backward()
    out["dx64"] = xl.grad.numpy()
    for n in R.NAMES:
        out["d64." + n] = getattr(eb, n).grad.numpy().copy()
    eb.zero_grad()
    v, like = eb(torch.from_numpy(x).double(), training=False)
    out["like64_eval"], out["v64_eval"] = like.detach().numpy(), v.detach().numpy()
    (like * gt).sum().backward()
    out["dmed64"] = eb.quantiles.grad[:, 0, 1].numpy().copy()
    for n in R.NAMES:
        out["d64_eval." + n] = getattr(eb, n).grad.numpy().copy()

    eb32 = module(torch.float32)
    with torch.no_grad():
        L32, _, _ = eb32._likelihood(as_cn(torch.from_numpy(x)))
    out["L32_written"] = back(L32).numpy()
    eb32.update()
    for k, t in eb32.state_dict().items():
        out["sd." + k] = t.detach().numpy()
    path = os.path.join(HERE, "g11_entropy_bottleneck.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
