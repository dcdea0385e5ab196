"""CPU: the weighted distortion of RDOQ, the curve and the budget search (include/flashgmm_amd.h section 3e) - the header declares
and the library exports the three _w calls and the two macros, the old layouts are unchanged; the Python surface and the refusals that
need no device; and, on the reference side alone (tests/rdo_weights_ref.py), that ones are the unweighted rule, that scaling every
weight by 4 at lambda is unit weights at lambda / 4, that J never rises, and the conditions that keep the GPU sweep of
tests/test_gpu_rdo_weights.py from passing vacuously, for every mode, clamped and not."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from tests import rdcurve_ref as V
from tests import rdo_weights_ref as W
from tests import rdoq_ref as Q
from tests import synth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["polya", "as", "logistic"]


def test_header_declares_and_library_exports_the_calls():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"#define FGMM_HAS_RDO_WEIGHTS 1\b", header) and re.search(r"#define FGMM_RDO_W_MAX 256\.0f\b", header) and "3e." in header
    assert re.search(r"typedef struct \{\s*const float \*chan_w;[^}]*const float \*pos_w;[^}]*\} fgmm_rdo_weights;", header)
    for name, tail in (("fgmm_gmc_rdoq_batch_w", r"double lambda,\s*const fgmm_rdo_weights \*w"),
                       ("fgmm_gmc_rdcurve_batch_w", r"const double \*lambdas, int n_lambda, const fgmm_rdo_weights \*w"),
                       ("fgmm_gmc_rdoq_budget_batch_w", r"fgmm_budget_result \*results[^,]*, const fgmm_rdo_weights \*w")):
        assert re.search(r"int\s+" + name + r"\s*\([^;]*" + tail + r"[^;]*\)\s*;", header), name
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name
    assert re.search(r"#define FGMM_ABI_VERSION\s+6\b", header)  # (not bumped: nothing existing changed)
    # the old layouts are what they were; the new struct is two pointers
    assert C.sizeof(_lib.fgmm_rdoq_item) == 128 and C.sizeof(_lib.fgmm_rdcurve_item) == 72 + 8 + 3 * 16 * 8 + 8 + 8
    assert C.sizeof(_lib.fgmm_budget_result) == 24 and C.sizeof(_lib.fgmm_rdo_weights) == 16
    assert [n for n, _ in _lib.fgmm_rdo_weights._fields_] == ["chan_w", "pos_w"] and _lib.FGMM_RDO_W_MAX == 256.0
    # the unweighted signatures have not moved
    assert len(_lib.SIGNATURES["fgmm_gmc_rdoq_batch"][1]) == 7 and len(_lib.SIGNATURES["fgmm_gmc_rdoq_batch_w"][1]) == 8
    assert len(_lib.SIGNATURES["fgmm_gmc_rdcurve_batch"][1]) == 8 and len(_lib.SIGNATURES["fgmm_gmc_rdoq_budget_batch"][1]) == 12


def test_invalid_arguments_are_refused_before_any_device_is_touched():
    L = _lib.lib()
    w = (_lib.fgmm_rdo_weights * 1)()
    assert L.fgmm_gmc_rdoq_batch_w(None, None, None, 0, 0, 1, -1.0, w) == 1 and b"lambda" in L.fgmm_last_error()
    assert L.fgmm_gmc_rdcurve_batch_w(None, None, None, 0, 0, 1, (C.c_double * 1)(0.5), 17, w) == 1 and b"n_lambda" in L.fgmm_last_error()
    assert L.fgmm_gmc_rdoq_budget_batch_w(None, None, None, 0, 0, 1, None, 0, None, 16.0, 9, None, w) == 1 and b"refine" in L.fgmm_last_error()


def test_python_surface_and_refusals():
    import flashgmm_amd
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    gmc = flashgmm_amd.GaussianMixtureConditional(K=4)
    for name in ("quantize_rdo", "quantize_rdo_batch", "rd_curve", "rd_curve_batch", "quantize_to_budget", "quantize_to_budget_batch"):
        ps = inspect.signature(getattr(gmc, name)).parameters
        for kw in ("channel_weights", "position_weights"):
            assert ps[kw].kind is inspect.Parameter.KEYWORD_ONLY and ps[kw].default is None, (name, kw)
    assert "weighted" in flashgmm_amd.RdCurve.__doc__.lower()
    y, s, m, w = (torch.from_numpy(a) for a in T.make_latent(3, 8, 4, 4))
    cw, pw = torch.ones(8), torch.ones(4, 4)
    bad = [dict(channel_weights=cw.double()), dict(position_weights=pw.half()), dict(channel_weights=cw[:7]), dict(channel_weights=cw.view(1, 8)),
           dict(position_weights=torch.ones(16)), dict(position_weights=torch.ones(1, 1, 4, 5)), dict(position_weights=torch.ones(1, 2, 4, 4)),
           dict(channel_weights=[1.0] * 8)]
    for kw in bad:  # refused for what the weights are, before the (CPU) latents are
        for call in (lambda **k: gmc.quantize_rdo(y, s, m, w, 0.5, **k), lambda **k: gmc.rd_curve(y, s, m, w, [0.5], **k),
                     lambda **k: gmc.quantize_to_budget(y, s, m, w, 100, **k)):
            with pytest.raises((TypeError, ValueError)):
                call(**kw)
    with pytest.raises((TypeError, ValueError)):  # one per item
        gmc.quantize_rdo_batch([y, y], [s, s], [m, m], [w, w], 0.5, position_weights=[pw])
    with pytest.raises((TypeError, ValueError)):  # stacked latents take [N, 1, h, w]
        gmc.quantize_rdo_batch(torch.cat([y, y]), torch.cat([s, s]), torch.cat([m, m]), torch.cat([w, w]), 0.5, position_weights=torch.ones(1, 1, 4, 4))
    with pytest.raises(RuntimeError, match="GPU only"):  # valid weights: the call goes on to what it refused before
        gmc.quantize_rdo(y, s, m, w, 0.5, channel_weights=cw, position_weights=pw)
    # the codecs
    c = GaussianMixtureConditionalLatentCodec(rdo_channel_weights=W.chan_w(8))
    assert c.rdo_channel_weights.dtype == torch.float32 and "rdo_channel_weights" in dict(c.named_buffers())
    assert GaussianMixtureConditionalLatentCodec().rdo_channel_weights is None
    with pytest.raises(ValueError):
        GaussianMixtureConditionalLatentCodec(rdo_channel_weights=torch.ones(2, 4))
    for name in ("coder_inputs_rdo", "coder_inputs_budget"):
        assert inspect.signature(getattr(c, name)).parameters["position_weights"].default is None
    for name in ("prepare", "compress"):
        assert inspect.signature(getattr(CheckerboardLatentCodec, name)).parameters["importance"].default is None
    # weights with fuse_head raise, as rdo_lambda does
    head = torch.nn.Conv2d(6, 3 * 4 * 8, 1)
    with pytest.raises(RuntimeError, match="fuse_head"):
        CheckerboardLatentCodec(latent_codec={"y": c}, entropy_parameters=head, fuse_head=True)
    fused = CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec()}, entropy_parameters=head, fuse_head=True)
    with pytest.raises(RuntimeError, match="fuse_head"):
        fused.compress(torch.zeros(1, 8, 4, 4), torch.zeros(1, 6, 4, 4), importance=torch.ones(1, 1, 4, 4))
    plain = CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec()}, rdo_lambda=0.5)
    for imp in (torch.ones(1, 1, 4, 5), torch.ones(1, 1, 4, 4).double()):
        with pytest.raises((TypeError, ValueError)):
            plain.compress(torch.zeros(1, 8, 4, 4), torch.zeros(1, 96, 4, 4), importance=imp)


def cases(clamp):
    return [(shape, seed, T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf)) for shape in Q.SHAPES for seed, zf in Q.SEEDS]


@pytest.fixture(scope="module")
def priced(oracle):
    """the GPU sweep's cases priced once: {(mode, clamp, shape, seed): (case, priced)}"""
    L = _lib.lib()
    return {(mode, clamp, shape, seed): (case, V.price(oracle, L, mode, *case, clamp=clamp))
            for mode in MODES for clamp in (True, False) for shape, seed, case in cases(clamp)}


def test_ones_are_the_unweighted_rule(oracle, priced):
    L = _lib.lib()
    for (mode, clamp, shape, seed), (case, p) in priced.items():
        M, hw = shape[0], shape[1] * shape[2]
        ones = W.weights_of(*case, np.ones(M, np.float32), np.ones(hw, np.float32), clamp=clamp)
        assert np.array_equal(ones, W.weights_of(*case, clamp=clamp)) and np.all(ones == 1.0)
        for lam in Q.LAMBDAS:
            want = Q.rdoq(oracle, L, mode, *case, lam, clamp=clamp)
            for kw in (dict(), dict(cw=np.ones(M, np.float32), pw=np.ones(hw, np.float32))):
                got = W.rdoq(oracle, L, mode, *case, lam, clamp=clamp, priced=p, **kw)
                for k in ("n_changed", "bits_q_before", "bits_q_after", "abs_max", "zero_bitmap", "n_coded", "n_away"):
                    assert got[k] == want[k], (mode, clamp, shape, seed, lam, k)
                assert Q.same_float_bits(got["y"], want["y"]) and np.array_equal(got["chan_after"], want["chan_after"])
                assert np.array_equal(got["symbols"], want["symbols"])
                assert got["j_before"].tobytes() == want["j_before"].tobytes() and got["j_after"].tobytes() == want["j_after"].tobytes()
        assert W.curve(p, Q.LAMBDAS, ones) == V.curve(p, Q.LAMBDAS)


def test_scaling_weights_and_lambda_together_changes_no_pick(oracle, priced):
    """4 * wt at lambda and wt at lambda / 4: both scalings are by powers of two, so J scales exactly and the picks are the same"""
    L = _lib.lib()
    for (mode, clamp, shape, seed), (case, p) in priced.items():
        M, hw = shape[0], shape[1] * shape[2]
        cw, pw = W.chan_w(M), W.pos_w(hw)
        for lam in (0.1, 0.5, 5.0):
            a = W.rdoq(oracle, L, mode, *case, lam, clamp=clamp, cw=cw * np.float32(4), pw=pw, priced=p)
            b = W.rdoq(oracle, L, mode, *case, lam / 4, clamp=clamp, cw=cw, pw=pw, priced=p)
            assert np.array_equal(a["pick"], b["pick"]) and a["bits_q_after"] == b["bits_q_after"], (mode, clamp, shape, seed, lam)
            u4 = W.rdoq(oracle, L, mode, *case, lam, clamp=clamp, cw=np.full(M, 4, np.float32), priced=p)
            u1 = W.rdoq(oracle, L, mode, *case, lam / 4, clamp=clamp, priced=p)  # (unit weights: rdoq_ref's own rule, by the test above)
            assert np.array_equal(u4["symbols"], u1["symbols"]), (mode, clamp, shape, seed, lam)


def test_j_never_rises_and_the_curve_is_rdoq_lambda_by_lambda(oracle, priced):
    L = _lib.lib()
    for (mode, clamp, shape, seed), (case, p) in priced.items():
        M, hw = shape[0], shape[1] * shape[2]
        cw, pw = W.chan_w(M), W.pos_w(hw)
        wt = W.weights_of(*case, cw, pw, clamp=clamp)
        c = W.curve(p, Q.LAMBDAS, wt)
        for j, lam in enumerate(Q.LAMBDAS):
            r = W.rdoq(oracle, L, mode, *case, lam, clamp=clamp, cw=cw, pw=pw, priced=p)
            ok = ~(np.isnan(r["j_before"]) | np.isnan(r["j_after"]))
            assert np.all(r["j_after"][ok] <= r["j_before"][ok]), (mode, clamp, shape, seed, lam)
            assert np.all((r["j_after"] < r["j_before"])[r["pick"] != 0])  # a move is a strict gain
            assert (c["bits_q_before"], c["bits_q_after"][j], c["n_changed"][j]) == (r["bits_q_before"], r["bits_q_after"], r["n_changed"])
            assert (c["ddist_q"][j] > 0) == (c["n_changed"][j] > 0)
        assert (c["bits_q_after"][0], c["n_changed"][0], c["ddist_q"][0]) == (c["bits_q_before"], 0, 0)  # lambda = 0


def test_the_fixed_weights_change_the_decisions(oracle, priced):
    """the non-vacuity conditions of the GPU sweep, at lambda = 0.5 with the fixed test weights, in EVERY case: the weighted choice
    differs from the unweighted one on at least 3 % of the coded latents; at least one latent moves only when weighted and at least
    one only when unweighted; channel-only and position-only weights each change at least one latent"""
    L = _lib.lib()
    for key, (case, p) in priced.items():
        mode, clamp, shape, seed = key
        M, hw = shape[0], shape[1] * shape[2]
        cw, pw = W.chan_w(M), W.pos_w(hw)
        kw = dict(clamp=clamp, priced=p)
        plain = W.rdoq(oracle, L, mode, *case, W.LAM, **kw)["pick"]
        both = W.rdoq(oracle, L, mode, *case, W.LAM, cw=cw, pw=pw, **kw)["pick"]
        n_diff = int((plain != both).sum())
        print(key, "coded", len(plain), "differ", n_diff, "only weighted", int(((both != 0) & (plain == 0)).sum()), "only unweighted",
              int(((both == 0) & (plain != 0)).sum()))
        assert len(plain) > 0 and n_diff * 100 >= 3 * len(plain), (key, n_diff, len(plain))
        assert ((both != 0) & (plain == 0)).any() and ((both == 0) & (plain != 0)).any(), key
        assert (W.rdoq(oracle, L, mode, *case, W.LAM, cw=cw, **kw)["pick"] != plain).any(), key
        assert (W.rdoq(oracle, L, mode, *case, W.LAM, pw=pw, **kw)["pick"] != plain).any(), key


def test_a_zero_weight_takes_the_cheapest_candidate(oracle, priced):
    L = _lib.lib()
    (case, p) = priced["polya", True, (12, 8, 13), 3]
    cw = W.chan_w(12)
    cw[1] = 0.0
    zb = T.to_coder_inputs(*case, clamp=True)[5]
    assert zb[1] == 1
    r = W.rdoq(oracle, L, "polya", *case, W.LAM, clamp=True, cw=cw, priced=p)
    rank = int(zb[:1].sum())
    sl = slice(rank * 104, (rank + 1) * 104)
    cm, c0, cp = (c[sl].astype(np.int64) for c in p["costs"])
    want = np.where(cm < c0, -1, 0)
    want = np.where(cp < np.minimum(cm, c0), 1, want)  # ties keep the earlier candidate
    assert np.array_equal(r["pick"][sl], np.where(p["cand"][sl], want, 0)) and (r["pick"][sl] != 0).any()
