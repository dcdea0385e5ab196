#!/usr/bin/env python3
"""Generate tests/golden/g10_likelihood.npz from the REAL reference: its own ``GaussianMixtureConditional(K=4)`` imported in place
(as make_golden.py does for G4), run on the CPU on the corpus of tests/like_ref.py - once in float64 (the module ``.double()``) and
once in float32, with autograd through the real ``LowerBound``.  Runs only where the reference is present; what is committed is data
plus this script.

The fixture, all in the public layout (y [1, 8, 16, 16], planes [1, 32, 16, 16]):
    y, scales, means, weights, g    the inputs, float32; g the fixed upstream gradient (both signs)
    like64_eval, like32_eval        ``forward(..., training=False)``: the bounded likelihood at round(y)
    L64, like64, like32             the mixture likelihood before the bound and after it, at v = y (no rounding, no noise): the class's
                                    own ``_likelihood`` and ``likelihood_lower_bound``, the two steps its forward runs after quantize
    dy64, dscales64, dmeans64, dweights64   autograd's gradients of sum(like64 * g), float64: thirteen planes
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
from tests import like_ref as R  # noqa: E402


def main():
    import torch

    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    GMC = mg.import_reference_entropy_models(O.ref_ans(""))
    y, sg, mu, pi, g = R.corpus()
    out = dict(y=y, scales=sg, means=mu, weights=pi, g=g)
    for dt, tag in ((torch.float64, "64"), (torch.float32, "32")):
        ref = GMC(K=4)
        ref = ref.double() if dt == torch.float64 else ref
        ref.eval()
        t = [torch.from_numpy(a).to(dt) for a in (y, sg, mu, pi)]
        with torch.no_grad():
            v, like = ref(*t, training=False)
        assert torch.equal(v, torch.round(t[0]))
        out["like" + tag + "_eval"] = like.numpy()
        leaves = [a.clone().requires_grad_(True) for a in t]
        L = ref._likelihood(*leaves)
        like = ref.likelihood_lower_bound(L)
        out["like" + tag] = like.detach().numpy()
        if dt == torch.float64:
            out["L64"] = L.detach().numpy()
            (like * torch.from_numpy(g).to(dt)).sum().backward()
            for name, leaf in zip(R.GRADS, leaves):
                out[name + "64"] = leaf.grad.numpy()
    path = os.path.join(HERE, "g10_likelihood.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
