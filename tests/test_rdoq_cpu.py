"""CPU: rate-distortion optimised quantisation (include/flashgmm_amd.h section 3c) - the header declares the call and the library
exports it; and, on the reference side alone (tests/rdoq_ref.py: the oracle's tables priced by the host's fgmm_symtab_bits, the
objective in float64), the properties the decision rule must have and the conditions that keep the GPU sweep of
tests/test_gpu_rdoq.py from passing vacuously, for every mode, clamped and not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flashgmm_amd import _lib
from tests import rdoq_ref as Q
from tests import synth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["polya", "as", "logistic"]


def test_header_declares_and_library_exports_the_call():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"int\s+fgmm_gmc_rdoq_batch\s*\(\s*fgmm_ctx\s*\*\s*ctx,\s*void\s*\*\s*stream,\s*fgmm_rdoq_item\s*\*\s*items,\s*int count,"
                     r"\s*int mode,\s*int clamp_scales,\s*double lambda\s*\)\s*;", header)
    assert "3c." in header and "fgmm_rdoq_item;" in header
    L = _lib.lib()
    assert hasattr(L, "fgmm_gmc_rdoq_batch") and L.fgmm_gmc_rdoq_batch.argtypes[-1] is C.c_double
    # the ctypes mirror has the header's layout: the input fields lead, as in fgmm_rate_item (one record dtype fills both)
    names = [n for n, _ in _lib.fgmm_rdoq_item._fields_]
    assert names == ["y", "params", "M", "K", "hw", "y_rdo", "zero_bitmap", "chan_bits_q_after", "abs_max", "status", "n_changed",
                     "bits_q_before", "bits_q_after"]
    assert [n for n, _ in _lib.fgmm_rate_item._fields_][:5] == names[:5] and C.sizeof(_lib.fgmm_rdoq_item) == 128


def test_invalid_arguments_are_refused_before_any_device_is_touched():
    """a bad lambda is FGMM_ERR_INVALID whatever else is passed (no context is needed to say so)"""
    L = _lib.lib()
    for lam in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert L.fgmm_gmc_rdoq_batch(None, None, None, 0, 0, 1, lam) == 1, lam
        assert b"lambda" in L.fgmm_last_error(), lam
    assert L.fgmm_gmc_rdoq_batch(None, None, None, 0, 0, 1, 0.5) == 1 and b"lambda" not in L.fgmm_last_error()  # (no context)


def test_python_surface():
    import flashgmm_amd
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    assert flashgmm_amd.RdoQuantized.__slots__ == ("y", "n_changed", "bits_q_before", "bits_q_after", "abs_max", "zero_bitmap", "channel_bits_q_after")
    gmc = flashgmm_amd.GaussianMixtureConditional(K=4)
    assert callable(gmc.quantize_rdo) and callable(gmc.quantize_rdo_batch)
    assert GaussianMixtureConditionalLatentCodec().rdo_lambda == 0.0 and GaussianMixtureConditionalLatentCodec(rdo_lambda=0.5).rdo_lambda == 0.5
    assert CheckerboardLatentCodec().rdo_lambda == 0.0
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            GaussianMixtureConditionalLatentCodec(rdo_lambda=bad)
        with pytest.raises(ValueError):
            CheckerboardLatentCodec(rdo_lambda=bad)
    import torch.nn as nn
    with pytest.raises(RuntimeError, match="fuse_head"):
        CheckerboardLatentCodec(entropy_parameters=nn.Conv2d(8, 48, 1), fuse_head=True, rdo_lambda=0.5)


@pytest.fixture(scope="module")
def sweep(oracle):
    """the reference over the GPU sweep's cases, computed once: {(mode, clamp, shape, seed, lam): result}"""
    L = _lib.lib()
    out = {}
    for mode in MODES:
        for clamp in (True, False):
            for shape in Q.SHAPES:
                for seed, zf in Q.SEEDS:
                    case = T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf)
                    for lam in Q.LAMBDAS:
                        out[mode, clamp, shape, seed, lam] = (case, Q.rdoq(oracle, L, mode, *case, lam, clamp=clamp))
    return out


def test_lambda_zero_changes_nothing(sweep):
    for (mode, clamp, shape, seed, lam), (case, r) in sweep.items():
        if lam == 0.0:
            want = np.round(case[0]) + np.float32(0.0)
            assert r["n_changed"] == 0 and r["bits_q_after"] == r["bits_q_before"] and Q.same_float_bits(r["y"], want), (mode, clamp, shape, seed)


def test_the_objective_never_rises(sweep):
    """J(chosen) <= J(round(y)) latent by latent, hence in sum; the result is integer-valued and within one step of round(y).
    (bits_q_after <= bits_q_before is NOT a property: a move may cost bits when distortion pays for it.)"""
    for key, (case, r) in sweep.items():
        assert np.all(r["j_after"] <= r["j_before"]), key
        assert float(r["j_after"].sum()) <= float(r["j_before"].sum()), key
        assert np.array_equal(r["y"], np.round(r["y"])) and np.all(np.abs(r["y"] - np.round(case[0])) <= 1), key
        assert r["bits_q_after"] == int(r["chan_after"].sum()), key


def test_conditions_that_keep_the_gpu_sweep_from_passing_vacuously(sweep):
    """for every mode, clamped and not: at lambda = 0.5 at least 5 % of the coded latents move in every case; over the sweep some move
    goes away from zero and some candidate is priced as a bypass escape"""
    for mode in MODES:
        for clamp in (True, False):
            away = byp = 0
            for (m, c, shape, seed, lam), (_, r) in sweep.items():
                if (m, c) != (mode, clamp):
                    continue
                away += r["n_away"]
                byp += r["n_bypass_cand"]
                if lam == 0.5:
                    assert r["n_changed"] * 20 >= r["n_coded"] > 0, (mode, clamp, shape, seed, r["n_changed"], r["n_coded"])
            assert away > 0 and byp > 0, (mode, clamp, away, byp)
