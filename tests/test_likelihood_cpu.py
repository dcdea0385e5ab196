"""CPU (-m "not gpu"): the entropy model's forward() (include/flashgmm_amd.h section 3g) as far as it can be checked without a GPU -
the header, the library's exports and the ctypes declarations; the float64 restatement the GPU tests measure against
(tests/like_ref.py), tied to the reference's own class through tests/golden/g10_likelihood.npz; and the corpus itself."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from tests import like_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("fgmm_gmc_likelihood_batch", "fgmm_gmc_likelihood_backward_batch")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g10_likelihood.npz")))


@pytest.fixture(scope="module")
def restated(gold):
    """the float64 restatement on the fixture's inputs, at v = y: (forward, backward at the fixture's g)"""
    t = [torch.from_numpy(gold[k]) for k in ("y", "scales", "means", "weights")]
    f = R.forward(*t, rnd=False, dtype=torch.float64)
    return f, R.backward(f, torch.from_numpy(gold["g"]))


def test_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_HAS_LIKELIHOOD 1\b", header, re.M) and " 3g. " in header
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M)
    L = _lib.lib()
    assert L.fgmm_abi_version() == 6
    raw = C.CDLL(_lib.LIB_PATH)
    for name in CALLS:
        assert name in header and hasattr(raw, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 7 and args[5:] == [C.c_float, C.c_float], name
    # the item structures begin with the fields the shared validation reads (fgmm_ctx.h LatentIn), at the rate item's offsets
    for struct in (_lib.fgmm_like_item, _lib.fgmm_like_grad_item):
        for field in ("y", "params", "M", "K", "hw"):
            assert getattr(struct, field).offset == getattr(_lib.fgmm_rate_item, field).offset, (struct.__name__, field)
    assert C.sizeof(_lib.fgmm_like_item) == 112 and C.sizeof(_lib.fgmm_like_grad_item) == 128


def test_restated_likelihood_and_decisions_equal_the_reference_in_float64(gold, restated):
    f, b = restated
    assert np.allclose(f["out"].numpy(), gold["like64"], rtol=1e-13, atol=0.0)
    assert np.allclose(f["L"].numpy(), gold["L64"], rtol=1e-13, atol=1e-300)
    for name in R.GRADS:
        # the pass-through decisions of the explicit formulas, row by row: a gradient the reference zeroes is zeroed, and the other way round
        assert np.array_equal(b[name].numpy() == 0, gold[name + "64"] == 0), name
    # ... and with rounding: the evaluation-mode likelihood
    t = [torch.from_numpy(gold[k]) for k in ("y", "scales", "means", "weights")]
    assert np.allclose(R.forward(*t, rnd=True, dtype=torch.float64)["out"].numpy(), gold["like64_eval"], rtol=1e-13, atol=0.0)
    # float32: the same operations in the same order on the same CPU
    assert np.array_equal(R.forward(*t, rnd=False)["out"].numpy(), gold["like32"])


def test_restated_gradients_equal_the_reference_in_float64(gold):
    """The float64 yardstick the GPU tests use for gradients (R.reference_gradients: autograd through the restated forward and the two
    restated pass-through rules) against the reference's own class: the likelihood to 1e-13 relative, every gradient to 1e-12 relative
    plus 1e-300 absolute, the pass-through decisions identical on every row.  (The explicit formulas of section 3g, R.backward, group
    the cancelling difference otherwise and cannot meet 1e-12 of the RESULT in float64: measured on this corpus up to 5.2e-11 for
    dscales, 5.5e-9 for dy, 2.4e-7 for dmeans, nearly all in regions (e) and (f).  What they do meet is the next test's.)"""
    t = [torch.from_numpy(gold[k]) for k in ("y", "scales", "means", "weights")]
    like, grads = R.reference_gradients(*t, torch.from_numpy(gold["g"]))
    assert np.allclose(like.numpy(), gold["like64"], rtol=1e-13, atol=0.0)
    for name in R.GRADS:
        got, want = grads[name].numpy(), gold[name + "64"]
        assert np.allclose(got, want, rtol=1e-12, atol=1e-300), name
        assert np.array_equal(got == 0, want == 0), name
    # with rounding nothing arrives at the latent, and the planes' gradients are those of the rounded values
    _, rounded = R.reference_gradients(*t, torch.from_numpy(gold["g"]), rnd=True)
    assert not rounded["dy"].any()
    _, at_v = R.reference_gradients(torch.round(t[0]), *t[1:], torch.from_numpy(gold["g"]))
    assert all(torch.equal(rounded[k], at_v[k]) for k in R.GRADS[1:])


def test_restated_gradients_equal_the_reference_up_to_their_cancellation(gold, restated):
    """What the explicit formulas of section 3g (R.backward, the kernel's arithmetic) and the reference's autograd agree to in float64: each
    deviates from the other by rounding errors of the terms that cancel, a few 2^-53 of their magnitudes.  Required here:
    |difference| <= 1e-12 * (the sum of the magnitudes of the terms the result is the difference of) - 4500 times the rounding unit, and
    still 1e5 times finer than binary32."""
    f, b = restated
    inv = 1.0 / np.sqrt(2.0 * np.pi)
    phi = lambda x: torch.exp(-0.5 * x * x) * inv  # noqa: E731
    gL = torch.abs(torch.where(b["pass_like"], torch.from_numpy(gold["g"]).double(), torch.zeros((), dtype=torch.float64))).unsqueeze(1)
    fu, fl, s, pi = phi(f["xu"]), phi(f["xl"]), f["s"], torch.abs(f["pi"])
    flat = lambda x: x.reshape(x.shape[0], -1, *x.shape[3:]).numpy()  # noqa: E731
    mag = {"dmeans": flat(gL * pi * (fu + fl) / s), "dscales": flat(gL * pi * (fu * torch.abs(f["xu"]) + fl * torch.abs(f["xl"])) / s),
           "dy": (gL * pi * (fu + fl) / s).sum(1).numpy(), "dweights": flat(gL * torch.abs(f["p"]))}
    for name in R.GRADS:
        assert np.all(np.abs(b[name].numpy() - gold[name + "64"]) <= 1e-12 * mag[name] + 1e-300), name


def test_corpus_has_what_it_claims(gold, restated):
    y, sg, mu, pi, g = R.corpus()
    for k, a in zip(("y", "scales", "means", "weights", "g"), (y, sg, mu, pi, g)):
        assert np.array_equal(a, gold[k]), k  # the fixture was made from this corpus
    yr = y.reshape(-1)
    rows = lambda a: a.reshape(4, -1).T  # noqa: E731  [2048, 4]
    sgr, mur, pir, gr = rows(sg), rows(mu), rows(pi), g.reshape(-1)
    L64 = gold["L64"].reshape(-1)
    sb = np.float32(R.SB)
    for name, (lo, hi) in R.REGIONS.items():
        assert hi - lo >= 128 and R.region_mask(name).sum() == hi - lo
    s = slice(*R.REGIONS["a"])
    assert np.all(np.abs(pir[s].sum(1) - 1) < 1e-6) and np.all(pir[s] > 0) and sgr[s].min() < 0.11 < 5 < sgr[s].max()
    s = slice(*R.REGIONS["b"])
    edges = {np.float32(0.02), np.nextafter(sb, np.float32(0)), sb, np.nextafter(sb, np.float32(1))}
    assert set(np.unique(sgr[s]).tolist()) == {float(e) for e in edges}
    G = restated[1]["dscales"].numpy().reshape(4, -1).T[s]  # (after the pass-through rule: positive ones survive only at sigma >= sb)
    assert (G > 0).any() and (G < 0).any() and (gr[s] > 0).any() and (gr[s] < 0).any()
    below = sgr[s] < sb
    assert np.all(G[below] <= 0) and (G[below] < 0).any() and (G[~below] > 0).any()
    s = slice(*R.REGIONS["c"])
    assert np.all(np.abs(yr[s, None].astype(np.float64) - mur[s]) >= 40.0 * sgr[s]) and np.all(L64[s] < 1e-9)
    assert (gr[s] > 0).any() and (gr[s] < 0).any()
    s = slice(*R.REGIONS["d"])
    hits = (mur[s] == yr[s, None]).sum(1)
    assert np.all(hits >= 1) and np.array_equal(np.round(yr[s]), yr[s])
    s = slice(*R.REGIONS["e"])
    assert sgr[s].min() >= 64 and sgr[s].max() <= 3000 and sgr[s].max() > 256
    s = slice(*R.REGIONS["f"])
    assert np.all(np.abs(sgr[s] / 256.0 - 1) <= 0.011) and np.all(np.abs(yr[s, None].astype(np.float64) - mur[s]) < 1)
    s = slice(*R.REGIONS["g"])
    sums = pir[s].astype(np.float64).sum(1)
    assert (np.abs(sums - 1.7) < 1e-5).sum() >= 64 and (pir[s].min(1) < 0).sum() >= 64
    # rows a float32 and a float64 evaluation may bound differently: at most 1 %, with and without rounding
    assert R.near_bound(gold["L64"]).mean() <= 0.01
    t = [torch.from_numpy(gold[k]) for k in ("y", "scales", "means", "weights")]
    assert R.near_bound(R.forward(*t, rnd=True, dtype=torch.float64)["L"].numpy()).mean() <= 0.01
