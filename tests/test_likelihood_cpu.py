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


# ---- what tests/test_gpu_likelihood_edges.py stands on -----------------------------------------------------------------------------------
def test_launch_form_table_and_every_instantiation():
    """``R.launch_form`` (LikeShape restated) on the table of cases: each lands on the form it is there for, and the two GPU modules
    together reach every (kernel, positions per lane, plane type, grid) the launcher's ladder can pick - 16 forward, 12 backward."""
    seen = set()
    for name, dts, items, fwd, bwd in R.CASES:
        for dt in dts:
            assert R.launch_form(items, dt != "f32", False) == fwd, (name, dt, "forward")
            assert R.launch_form(items, dt != "f32", True) == bwd, (name, dt, "backward")
        seen |= {(back, form[0], dt, form[1]) for dt in dts for back, form in ((False, fwd), (True, bwd))}
    every = {(back, vec, dt, lin) for back in (False, True) for dt in R.ALL for lin in (True, False)
             for vec in ((1, 4) if back or dt == "f32" else (1, 4, 8))}
    assert len(every) == 28 and seen == every, sorted(every - seen)
    new = {(back, form[0], dt, form[1]) for name, dts, _, fwd, bwd in R.CASES if not name.startswith("old_") for dt in dts
           for back, form in ((False, fwd), (True, bwd))}
    assert {(back, 1, dt, lin) for back in (False, True) for dt in R.TWO for lin in (True, False)} <= new  # the eight the old module leaves out
    # the decisions one by one
    it = R.dense_item
    assert R.launch_form([it(2, 512)], True, False) == (8, True) and R.launch_form([it(2, 512)], True, True) == (4, True)  # the backward cap
    assert R.launch_form([it(2, 512), it(2, 256)], True, False) == (4, True)      # 8 -> 4: one item does not fill 8, all fill 4
    assert R.launch_form([it(2, 512), it(2, 264)], True, False) == (8, False)     # ... 4 would not keep the linear grid either: 8 stays
    assert R.launch_form([it(2, 512), it(2, 260)], True, False) == (4, False)     # hw % 8 != 0
    assert R.launch_form([it(2, 512)], False, False) == (4, True)                 # float32 planes have no 8
    assert R.launch_form([it(2, 512, planes_off=8)], True, False) == (4, True)    # two-byte planes at 8 bytes: 4 yes, 8 no
    assert R.launch_form([it(2, 512, planes_off=8)], False, False) == (1, True)
    assert R.launch_form([it(2, 512, planes_off=4)], True, False) == (1, True)
    assert R.launch_form([it(2, 512, stride_c=516)], True, False) == (4, True) and R.launch_form([it(2, 512, stride_c=514)], True, False) == (1, True)
    assert R.launch_form([it(2, 512), it(1, 64, rest_off=(0, 0, 8))], False, True) == (1, True)  # one output of one item
    assert R.launch_form([it(2, 512), it(1, 32)], False, False) == (4, False) and R.launch_form([it(2, 512), it(0, 0)], False, False) == (4, True)


def test_g_from_bits_and_its_left_out_rule():
    out = torch.tensor([0.25, 1e-9, 2.0, 0.0, -0.5, float("inf"), float("nan")], dtype=torch.float32)
    ln2 = np.float32(R.LN2F)
    for gb in (1.5, -0.375):
        got = R.g_from_bits(out, gb).numpy()
        want = [-np.float32(gb) / (np.float32(x) * ln2) for x in (0.25, 1e-9, 2.0)] + [0.0] * 4
        assert got.dtype == np.float32 and np.array_equal(got, np.array(want, np.float32)), gb
    assert R.counts(out).tolist() == [True, True, True, False, False, False, False]


def test_edge_inputs_are_the_corpus_with_planted_latents():
    y, sg, mu, pi, g, planted = R.edge_inputs()
    plain = R.corpus()
    assert [k for k, _, _ in planted[:len(R.KINDS)]] == list(R.KINDS) and set(R.KINDS) >= {
        "nan_sigma", "nan_weight", "y_pinf", "y_ninf", "mu_pinf", "y_mu_pinf", "sigma_pinf", "sigma_zero"}
    rows = [i for _, i, _ in planted]
    assert len(set(rows)) == len(rows)
    in_region = lambda i, r: R.REGIONS[r][0] <= i < R.REGIONS[r][1]  # noqa: E731
    for kind in R.KINDS:
        at = [i for k, i, _ in planted if k == kind]
        assert sum(in_region(i, "a") for i in at) >= 4 and sum(in_region(i, "e") for i in at) >= 4 and all(in_region(i, "a") or in_region(i, "e") for i in at)
    hole = R.planted_mask(planted)
    assert hole.sum() == len(rows)
    for a, b in zip((y, sg, mu, pi, g), plain):
        m = hole if a.shape[1] == 8 else np.tile(hole, (1, 4, 1, 1))
        assert np.array_equal(a[~m], b[~m]) and a.dtype == np.float32
    assert np.array_equal(g, plain[4])
    # what is planted is what the list says, and bfloat16 holds it
    for kind, i, k in planted:
        s_, m_, p_ = (a.reshape(4, -1)[k, i] for a in (sg, mu, pi))
        yi = y.reshape(-1)[i]
        ok = {"nan_sigma": np.isnan(s_), "nan_weight": np.isnan(p_), "y_pinf": yi == np.inf, "y_ninf": yi == -np.inf, "mu_pinf": m_ == np.inf and np.isfinite(yi),
              "y_mu_pinf": yi == np.inf and m_ == np.inf, "sigma_pinf": s_ == np.inf, "sigma_zero": s_ == 0, "weight_pinf": p_ == np.inf}[kind]
        assert ok, (kind, i, k)
    # every class of likelihood turns up: NaN, +inf, and finite
    out = R.forward(*(torch.from_numpy(a) for a in (y, sg, mu, pi)), rnd=False)["out"]
    assert set(R.classes(out)[hole].tolist()) == {0, 1, 4} and int((~R.counts(out)).sum()) == int((R.classes(out) != 4).sum()) > 0


@pytest.mark.parametrize("rnd", [False, True])
def test_select_and_mask_multiply_differ_where_a_non_finite_gradient_is_not_passed(rnd):
    """Section 3g selects (`rule ? G : 0`), the reference multiplies (`mask * G`, bound_ops.py:40-42): a NaN or +inf G_k that the rule
    does not pass is 0 in the one and NaN in the other.  On the planted latents of the issue's eight kinds, in binary32, the classes of
    the restated formulas (R.backward) and of autograd through the reference's operations (R.reference_gradients) differ at exactly
    those elements of dscales, and nowhere in dy, dmeans and dweights.  (A +inf weight is left out here: the two group phi / s
    differently, and inf - inf is NaN in one of them only.)"""
    y, sg, mu, pi, g, planted = R.edge_inputs()
    t = [torch.from_numpy(a) for a in (y, sg, mu, pi, g)]
    b = R.backward(R.forward(*t[:4], rnd=rnd), t[4])
    _, ref = R.reference_gradients(*t, rnd=rnd, dtype=torch.float32)
    hole = R.planted_mask([p for p in planted if p[0] != "weight_pinf"])
    dropped = ~b["pass_scale"].numpy() & ~np.isfinite(b["G"].numpy())
    assert dropped[np.tile(hole, (1, 4, 1, 1))].sum() >= 8 and not dropped[~np.tile(R.planted_mask(planted), (1, 4, 1, 1))].any()
    assert torch.isfinite(t[4]).all()  # (the other select, gL, never meets a non-finite g here: a left-out latent's g is 0, not NaN)
    for name in R.GRADS:
        m = hole if name == "dy" else np.tile(hole, (1, 4, 1, 1))
        differ = (R.classes(b[name]) != R.classes(ref[name])) & m
        assert np.array_equal(differ, dropped & m if name == "dscales" else np.zeros_like(m)), name
        if name == "dscales":
            assert np.all(b[name].numpy()[differ] == 0) and np.all(np.isnan(ref[name].numpy()[differ]))


@pytest.mark.parametrize("sb,lb", R.BOUNDS)
def test_corpus_at_other_bounds(sb, lb):
    y, sg, mu, pi, g = R.corpus(sb=sb)
    plain = R.corpus()
    b = R.plane_mask("b")  # (region (b)'s latents and means are drawn around its sigmas; every other region is the corpus's)
    assert np.array_equal(y[~R.region_mask("b")], plain[0][~R.region_mask("b")]) and np.array_equal(g, plain[4])
    assert all(np.array_equal(a[~b], p[~b]) for a, p in zip((sg, mu, pi), plain[1:4]))
    sb32 = np.float32(sb)
    assert set(np.unique(sg[b]).tolist()) == {float(np.float32(0.02 * (sb / R.SB))), float(np.nextafter(sb32, np.float32(0))), float(sb32),
                                              float(np.nextafter(sb32, np.float32(1)))}
    t = [torch.from_numpy(a) for a in (y, sg, mu, pi)]
    for rnd in (False, True):  # rows a float32 and a float64 evaluation may bound differently: at most 1 %
        L = R.forward(*t, rnd=rnd, sb=sb, lb=lb, dtype=torch.float64)["L"].numpy()
        assert (~R.near_bound(L, lb)).mean() >= 0.99, (sb, lb, rnd)
    f = R.forward(*t, rnd=False, sb=sb, lb=lb)
    L = f["L"].numpy()
    if lb == 0:  # what is left out of the rate: region (c)'s exact zeros and region (g)'s negative L; and every gradient passes
        assert np.array_equal(f["out"].numpy(), L) and np.all(L[R.region_mask("c")] == 0) and (L[R.region_mask("g")] < 0).sum() >= 8
        assert R.backward(f, torch.from_numpy(g))["pass_like"].all()
        # (in region (c) every p_k is exactly 0 in binary32, so no gradient there can show a pass-through decision: all are 0 * g)
        assert not f["p"].numpy()[0][:, R.region_mask("c")[0]].any()
    if lb == 0.5:
        assert (L[R.region_mask("a")] < np.float32(0.5)).mean() > 0.5
