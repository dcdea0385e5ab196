#!/usr/bin/env python3
"""Generate tests/golden/g12_eb_update.npz from the REAL reference: its own ``EntropyBottleneck`` imported in place (as make_golden_eb.py
does for G11), on the CPU, with the parameters of the six channels of tests/eb_ref.py's corpus loaded into it, after
``update(force=True, update_quantiles=True)`` in float32; and its quantile search once more on the module in float64.  Runs only where
the reference is present; what is committed is data plus this script.

The fixture:
    p.<name>            the parameters, float32 (those of g11)
    sd.<key>            the float32 module's state dict after the update: quantiles [6, 1, 3], _offset, _quantized_cdf, _cdf_length
    q64                 the float64 module's ``_search_target`` on the three targets [6, 3] (the reference's own stopping rule: all
                        channels pass isclose(rtol 1e-4, atol 1e-3))
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

    _, p, _, _, _ = R.corpus()
    out = {"p." + n: p[n] for n in R.NAMES}

    def module(dtype):
        eb = EntropyBottleneck(R.C)
        with torch.no_grad():
            for n in R.NAMES:
                getattr(eb, n).copy_(torch.from_numpy(p[n]))
        return eb.to(dtype).eval()

    eb32 = module(torch.float32)
    assert eb32.update(force=True, update_quantiles=True)
    for k, t in eb32.state_dict().items():
        out["sd." + k] = t.detach().numpy()
    eb64 = module(torch.float64)
    with torch.no_grad():  # _update_quantiles makes its bounds in float32: its body, with float64 bounds (:573-588)
        low, high = (torch.full((R.C, 1, 1), v, dtype=torch.float64) for v in (-1e5, 1e5))
        f = lambda y: eb64._logits_cumulative(y, stop_gradient=True)  # noqa: E731
        q = [eb64._search_target(f, eb64.target[i], low, high, 1e-4, 1e-3)[:, 0, 0] for i in range(3)]
    out["q64"] = torch.stack(q, 1).numpy()
    path = os.path.join(HERE, "g12_eb_update.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; pmf_length", (out["sd._cdf_length"] - 2).tolist())


if __name__ == "__main__":
    main()
