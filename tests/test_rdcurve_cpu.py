"""CPU: the rate-distortion curve and the budget search (include/flashgmm_amd.h section 3d) - the header declares the calls and the
library exports them; and, on the reference side alone (tests/rdcurve_ref.py), that the curve is tests/rdoq_ref.py's RDOQ lambda by
lambda and the conditions that keep the GPU sweep of tests/test_gpu_rdcurve.py from passing vacuously, for every mode, clamped and not."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from flashgmm_amd import _lib
from tests import rdcurve_ref as V
from tests import rdoq_ref as Q
from tests import synth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["polya", "as", "logistic"]


def test_header_declares_and_library_exports_the_calls():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert "#define FGMM_HAS_RDCURVE 1" in header and "3d." in header and re.search(r"#define FGMM_RDCURVE_MAX 16\b", header)
    assert re.search(r"int\s+fgmm_gmc_rdcurve_batch\s*\(\s*fgmm_ctx\s*\*\s*ctx,\s*void\s*\*\s*stream,\s*fgmm_rdcurve_item\s*\*\s*items,\s*int count,"
                     r"\s*int mode,\s*int clamp_scales,\s*const double\s*\*\s*lambdas,\s*int n_lambda\s*\)\s*;", header)
    assert re.search(r"int\s+fgmm_gmc_rdoq_budget_batch\s*\(", header) and re.search(r"FGMM_BUDGET_UNMET = 7\b", header)
    assert re.search(r"#define FGMM_ABI_VERSION\s+\d+", header)  # (not bumped: nothing existing changed)
    L = _lib.lib()
    assert hasattr(L, "fgmm_gmc_rdcurve_batch") and hasattr(L, "fgmm_gmc_rdoq_budget_batch")
    assert _lib.FGMM_RDCURVE_MAX == V.N_MAX == 16 and _lib.FGMM_BUDGET_UNMET == V.BUDGET_UNMET
    names = [n for n, _ in _lib.fgmm_rdcurve_item._fields_]
    assert names[:5] == [n for n, _ in _lib.fgmm_rate_item._fields_][:5]  # inputs as fgmm_rate_item
    assert names[5:] == ["bits_q_before", "bits_q_after", "n_changed", "ddist_q", "n_symbols", "status", "pad_"]
    assert C.sizeof(_lib.fgmm_rdcurve_item) == 72 + 8 + 3 * 16 * 8 + 8 + 8 and C.sizeof(_lib.fgmm_budget_result) == 24


def test_invalid_arguments_are_refused_before_any_device_is_touched():
    L = _lib.lib()
    lam = (C.c_double * 17)(*([0.5] * 17))
    for n in (0, 17, -1):
        assert L.fgmm_gmc_rdcurve_batch(None, None, None, 0, 0, 1, lam, n) == 1 and b"n_lambda" in L.fgmm_last_error(), n
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.fgmm_gmc_rdcurve_batch(None, None, None, 0, 0, 1, (C.c_double * 2)(0.5, bad), 2) == 1 and b"lambda[1]" in L.fgmm_last_error()
    for lmax in (0.0, -1.0, float("nan"), float("inf")):
        assert L.fgmm_gmc_rdoq_budget_batch(None, None, None, 0, 0, 1, None, 0, None, lmax, 2, None) == 1 and b"lambda_max" in L.fgmm_last_error()
    for refine in (-1, 9):
        assert L.fgmm_gmc_rdoq_budget_batch(None, None, None, 0, 0, 1, None, 0, None, 16.0, refine, None) == 1 and b"refine" in L.fgmm_last_error()


def test_python_surface():
    import flashgmm_amd
    from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec

    gmc = flashgmm_amd.GaussianMixtureConditional(K=4)
    for name in ("rd_curve", "rd_curve_batch", "quantize_to_budget", "quantize_to_budget_batch"):
        assert callable(getattr(gmc, name)), name
    c = flashgmm_amd.RdCurve([0.0, 0.5], 100 << 24, [100 << 24, 40 << 24], [0, 7], [0, 3 << 31])
    assert c.lambdas == (0.0, 0.5) and c.bits_after == (100.0, 40.0) and c.nbytes == (20, 12) and c.distortion_added == (0.0, 1.5)
    # a budget result is an RdoQuantized with four more fields; a plain one is constructed as before and reads them as None
    assert issubclass(flashgmm_amd.BudgetQuantized, flashgmm_amd.RdoQuantized)
    q = flashgmm_amd.RdoQuantized(None, 1, 2, 3, 4, None)
    assert (q.lam, q.bytes_pred, q.budget_met, q.passes) == (None, None, None, None)
    b = flashgmm_amd.BudgetQuantized(None, 1, 2, 3, 4, None, None, 0.25, 100, True, 3)
    assert (b.n_changed, b.lam, b.bytes_pred, b.budget_met, b.passes) == (1, 0.25, 100, True, 3)
    assert GaussianMixtureConditionalLatentCodec().target_bytes is None and GaussianMixtureConditionalLatentCodec(target_bytes=100).target_bytes == 100
    with pytest.raises(ValueError):
        GaussianMixtureConditionalLatentCodec(target_bytes=100, rdo_lambda=0.5)
    with pytest.raises(ValueError):
        GaussianMixtureConditionalLatentCodec(target_bytes=-1)


def cases(clamp):
    return [(shape, seed, T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf)) for shape in Q.SHAPES for seed, zf in Q.SEEDS]


@pytest.fixture(scope="module")
def priced(oracle):
    """the GPU sweep's cases priced once: {(mode, clamp, shape, seed): (case, priced)}"""
    L = _lib.lib()
    return {(mode, clamp, shape, seed): (case, V.price(oracle, L, mode, *case, clamp=clamp))
            for mode in MODES for clamp in (True, False) for shape, seed, case in cases(clamp)}


def test_the_curve_is_rdoq_lambda_by_lambda(oracle, priced):
    L = _lib.lib()
    for (mode, clamp, shape, seed), (case, p) in priced.items():
        c = V.curve(p, Q.LAMBDAS)
        for j, lam in enumerate(Q.LAMBDAS):
            r = Q.rdoq(oracle, L, mode, *case, lam, clamp=clamp)
            assert (c["bits_q_before"], c["bits_q_after"][j], c["n_changed"][j]) == (r["bits_q_before"], r["bits_q_after"], r["n_changed"]), (mode, clamp, shape, seed, lam)
            assert (c["ddist_q"][j] > 0) == (c["n_changed"][j] > 0), (mode, clamp, shape, seed, lam)
        assert (c["bits_q_after"][0], c["n_changed"][0], c["ddist_q"][0]) == (c["bits_q_before"], 0, 0)  # lambda = 0
        assert max(c["n_changed"]) > 0


@pytest.fixture(scope="module")
def priced_budget(oracle):
    """the budget tests' cases (rdcurve_ref.BUDGET_CASES) priced once: {(mode, clamp): [priced]}"""
    L = _lib.lib()
    return {(mode, clamp): [V.price(oracle, L, mode, *case, clamp=clamp) for case in V.budget_cases(clamp)] for mode in MODES for clamp in (True, False)}


def test_the_search_brackets_the_budget(priced_budget):
    """for each case bytes(0) > bytes(16); with the budget half way between (a multiple of 4) the search ends inside (0, 16), on a
    feasible point whose predecessor in the final grid is not, and at least one refinement round moved hi"""
    L = _lib.lib()
    for key, ps in priced_budget.items():
        for i, p in enumerate(ps):
            f = V.group_f(L, [p])
            b0, b16 = f([0.0, 16.0])
            assert b0 > b16, (key, i)
            budget = V.budget_of(b0, b16)
            r = V.search(f, budget)
            assert 0.0 < r["lam"] < 16.0 and r["status"] == 0 and r["passes"] == 3, (key, i, r)
            assert r["bytes_pred"] <= budget < r["f_before"], (key, i, r, budget)
            assert r["bytes_pred"] == f([r["lam"]])[0] and r["moved"] >= 1, (key, i, r)
            assert V.search(f, budget, refine=0)["passes"] == 1


def test_the_unmet_and_the_already_fits_branches(priced_budget):
    L = _lib.lib()
    group = priced_budget["polya", True]
    f = V.group_f(L, [group[2]])
    b0, b16 = f([0.0, 16.0])
    r = V.search(f, 8)  # a non-empty item never fits the empty stream's 8 bytes
    assert b16 > 8 and (r["lam"], r["status"], r["bytes_pred"], r["passes"]) == (16.0, V.BUDGET_UNMET, b16, 1)
    r = V.search(f, b0)  # round(y) already fits: j* = 0
    assert (r["lam"], r["status"], r["bytes_pred"], r["passes"]) == (0.0, 0, b0, 1)
    # one group of all eight cases: the same bracket on the sum
    for key, group in priced_budget.items():
        f = V.group_f(L, group)
        b0, b16 = f([0.0, 16.0])
        r = V.search(f, V.budget_of(b0, b16))
        assert len(group) == 8 and 0.0 < r["lam"] < 16.0 and r["moved"] >= 1 and r["bytes_pred"] <= V.budget_of(b0, b16) < r["f_before"], (key, r)
