"""CPU (-m "not gpu"): the likelihood from the parameter head's logits (include/flashgmm_amd.h section 3h) as far as it can be checked
without a GPU - the header, the library's exports and the ctypes declarations; the derivative of the softmax over K as section 3h
states it (tests/like_logits_ref.py) against autograd in float64 and against torch's own softmax backward in float32; the logits
corpus; the Python surface; and the table of cases tests/test_gpu_likelihood_logits.py runs the 28 instantiations of the logits form
with."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec
from tests import like_logits_ref as Q
from tests import like_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"fgmm_gmc_likelihood_logits_batch": "fgmm_gmc_likelihood_batch", "fgmm_gmc_likelihood_logits_backward_batch": "fgmm_gmc_likelihood_backward_batch"}

# The cases of tests/test_gpu_likelihood_logits.py::test_every_instantiation_of_the_logits_form, by name in R.CASES: (case, plane type).
# Together their forward and backward launch forms are all 28 instantiations (test_the_chosen_cases_reach_all_28 below).
INSTANTIATION_CASES = [
    ("old_corpus", "f32"), ("old_hw255", "f32"), ("old_B3_hw64", "f32"), ("old_offset_hw256", "f32"),
    ("old_hw256", "f16"), ("old_hw256", "bf16"), ("old_hw264", "f16"), ("old_hw264", "bf16"), ("old_hw252", "f16"), ("old_hw252", "bf16"),
    ("old_hw512", "f16"), ("old_hw512", "bf16"), ("a_hw35", "f16"), ("a_hw35", "bf16"), ("a_planes_off", "f16"), ("a_planes_off", "bf16"),
    ("b_unequal", "f32"), ("b_unequal", "bf16"), ("b_M0", "f32"), ("b_hw0", "bf16"), ("c_chunk_hw64", "f32"), ("c_chunk_hw64", "bf16"),
    ("c_chunk_hw35", "f32"),
]


def test_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_HAS_LIKELIHOOD_LOGITS 1\b", header, re.M) and " 3h. " in header
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M)
    L = _lib.lib()
    assert L.fgmm_abi_version() == 6
    raw = C.CDLL(_lib.LIB_PATH)
    for name, plain in CALLS.items():
        assert name in header and hasattr(raw, name), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[plain], name  # 3g's argument lists
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == 7 and args[5:] == [C.c_float, C.c_float], name
    assert _lib.SIGNATURES["fgmm_gmc_likelihood_logits_batch"][1][2] == C.POINTER(_lib.fgmm_like_item)
    assert _lib.SIGNATURES["fgmm_gmc_likelihood_logits_backward_batch"][1][2] == C.POINTER(_lib.fgmm_like_grad_item)
    assert C.sizeof(_lib.fgmm_like_item) == 112 and C.sizeof(_lib.fgmm_like_grad_item) == 128


@pytest.fixture(scope="module")
def corpus64():
    """the logits corpus in float64 at v = y: (tensors, pi64, R.forward, R.backward at the corpus's g)"""
    t = [torch.from_numpy(a) for a in Q.logits_corpus()]
    pi = Q.softmax_planes(t[3])
    f = R.forward(t[0], t[1], t[2], pi, rnd=False, dtype=torch.float64)
    return t, pi, f, R.backward(f, t[4])


def test_derivative_in_float64_equals_autograd_up_to_its_cancellation(corpus64):
    """section 3h's three lines on float64 tensors, at 3g's dweights (R.backward), against autograd through torch.softmax and the restated
    forward: |difference| <= 1e-12 * mag + 1e-300 on every row, mag the magnitude of the terms dl_k is the difference of - the form of
    tests/test_likelihood_cpu.py's cancellation test (dweights itself meets 1e-12 of its own magnitude |gL * p_k| there, which mag holds
    pi_k times over)."""
    t, pi, f, b = corpus64
    got = Q.dlogits(pi, b["dweights"])
    _, ref = Q.reference_gradients_logits(*t)
    m = Q.mag(pi, b["dweights"])
    assert got.dtype == torch.float64 and got.shape == t[3].shape
    assert torch.all(torch.abs(got - ref["dweights"]) <= 1e-12 * m + 1e-300)
    assert float(torch.abs(ref["dweights"]).max()) > 0
    for name in ("dy", "dscales", "dmeans"):  # the rest of the backward is 3g's, on that pi: the same autograd
        assert torch.equal(ref[name], R.reference_gradients(t[0], t[1], t[2], pi, t[4])[1][name]), name


def test_derivative_in_float32_equals_torch_s_softmax_backward(corpus64):
    """float32: softmax then ``dlogits`` composed by hand against torch's own softmax backward at the same pi and the same dpi.  Both
    are a handful of binary32 operations on terms no larger than mag: four products and three additions for t (each at most half an
    ulp of a partial sum <= sum_j pi_j |dpi_j|), one subtraction, one product - under 8 * 2^-24 * mag for either, whatever the order
    and the contraction torch's kernel uses, so 16 * 2^-24 * mag between the two (plus the smallest normal binary32 absolute)."""
    t, _, _, _ = corpus64
    pi = Q.softmax_planes(t[3], torch.float32)
    f = R.forward(t[0], t[1], t[2], pi, rnd=False)
    dpi = R.backward(f, t[4])["dweights"]
    assert pi.dtype == dpi.dtype == torch.float32
    got = Q.dlogits(pi, dpi)
    want = torch._softmax_backward_data(R._k(dpi), R._k(pi), 1, torch.float32).reshape(pi.shape)
    m = Q.mag(pi, dpi)
    assert got.dtype == torch.float32 and torch.all(torch.abs(got.double() - want.double()) <= 16 * 2.0 ** -24 * m + 2.0 ** -126)
    # ... and the composition is a derivative at all: against autograd through torch.softmax in float32 by the same rule
    lg = t[3].clone().requires_grad_(True)
    Q.softmax_planes(lg, torch.float32).backward(dpi)
    assert torch.all(torch.abs(got.double() - lg.grad.double()) <= 16 * 2.0 ** -24 * m + 2.0 ** -126)


def test_logits_corpus_has_what_it_claims(corpus64):
    y, sg, mu, lg, g = Q.logits_corpus()
    plain = R.corpus()
    assert all(np.array_equal(a, b) for a, b in zip((y, sg, mu, g), (plain[0], plain[1], plain[2], plain[4])))
    assert lg.dtype == np.float32 and lg.shape == plain[3].shape
    rows = Q.logit_rows(lg)
    d = rows - rows.max(1, keepdims=True)  # binary32, as softmax4 forms it
    s = slice(*R.REGIONS["b"])
    assert np.all(((d[s] < -41.0).sum(1) == 1) & (((d[s] > -41.0) & (d[s] <= -40.0)).sum(1) == 1))
    s = slice(*R.REGIONS["d"])
    assert np.all(rows[s] == rows[s, :1])
    s = slice(*R.REGIONS["e"])
    top2 = np.sort(rows[s], 1)
    assert np.all(top2[:, 3] - top2[:, 2] >= 20.0)
    s = slice(*R.REGIONS["f"])
    assert np.all(np.abs(rows[s]) >= 70.0) and (rows[s] > 0).any() and (rows[s] < 0).any()
    for name in "acg":
        s = slice(*R.REGIONS[name])
        assert np.abs(rows[s]).max() < 12 and 1.5 < rows[s].std() < 2.5
    # rows a float32 and a float64 evaluation may bound differently: at most 1 %, with and without rounding
    t, pi, f, _ = corpus64
    assert R.near_bound(f["L"].numpy()).mean() <= 0.01
    assert R.near_bound(R.forward(t[0], t[1], t[2], pi, rnd=True, dtype=torch.float64)["L"].numpy()).mean() <= 0.01


def test_planted_non_finite_logits():
    y, sg, mu, lg, g, planted = Q.nonfinite_logits()
    plain = Q.logits_corpus()
    rows, before = Q.logit_rows(lg), Q.logit_rows(plain[3])
    at = [i for _, i, _ in planted]
    assert len(set(at)) == len(at) == 16 and all(R.REGIONS["a"][0] <= i < R.REGIONS["a"][1] for i in at)
    assert all(sum(k == kind for k, _, _ in planted) == 4 for kind in Q.LOGIT_KINDS)
    hole = np.zeros(2048, bool)
    hole[at] = True
    assert np.array_equal(rows[~hole], before[~hole]) and all(np.array_equal(a, b) for a, b in zip((y, sg, mu, g), (plain[0], plain[1], plain[2], plain[4])))
    for kind, i, k in planted:
        ok = {"nan": np.isnan(rows[i, k]) and np.isfinite(np.delete(rows[i], k)).all(), "pinf": rows[i, k] == np.inf,
              "ninf": rows[i, k] == -np.inf and np.isfinite(np.delete(rows[i], k)).all(), "all_ninf": np.all(rows[i] == -np.inf)}[kind]
        assert ok, (kind, i, k)


def test_python_surface():
    with pytest.raises(ValueError):
        GaussianMixtureConditionalLatentCodec(K=4, quantizer="weighted_mean_ste", fuse_forward_softmax=True)
    assert GaussianMixtureConditionalLatentCodec(K=4, fuse_forward_softmax=True).fuse_forward_softmax is True
    assert GaussianMixtureConditionalLatentCodec(K=4).fuse_forward_softmax is False
    assert GaussianMixtureConditionalLatentCodec(K=4, quantizer="weighted_mean_ste").fuse_forward_softmax is False
    assert inspect.signature(GaussianMixtureConditionalLatentCodec.__init__).parameters["fuse_forward_softmax"].default is False
    for name in ("likelihood", "forward", "rate_bits"):
        p = inspect.signature(getattr(GaussianMixtureConditional, name)).parameters["weights_are_logits"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, name
    p = inspect.signature(GaussianMixtureConditional.forward_params).parameters
    assert list(p) == ["self", "inputs", "params", "training"] and p["training"].default is None
    p = inspect.signature(GaussianMixtureConditional.rate_bits_params).parameters
    assert list(p) == ["self", "inputs", "params", "training", "return_nonfinite"] and p["training"].default is None
    assert p["return_nonfinite"].default is False and p["return_nonfinite"].kind is inspect.Parameter.KEYWORD_ONLY


def test_the_chosen_cases_reach_all_28():
    """every (pass, positions per lane, plane type, grid) of the launcher's ladder is the forward or the backward form of a chosen case"""
    seen = set()
    for name, dt in INSTANTIATION_CASES:
        fwd, bwd = R.FORMS[name, dt]
        seen |= {(False, fwd[0], dt, fwd[1]), (True, bwd[0], dt, bwd[1])}
    every = {(back, vec, dt, lin) for back in (False, True) for dt in R.ALL for lin in (True, False)
             for vec in ((1, 4) if back or dt == "f32" else (1, 4, 8))}
    assert len(every) == 28 and seen == every, sorted(every - seen)
    names = {n for n, _ in INSTANTIATION_CASES}
    assert {"b_unequal", "b_M0", "b_hw0", "c_chunk_hw64", "c_chunk_hw35"} <= names  # unequal items, an empty item of either kind, chunk views
