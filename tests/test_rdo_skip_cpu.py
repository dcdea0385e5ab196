"""CPU: channel skipping for RDOQ, the curve and the budget search (include/flashgmm_amd.h section 3f) - the header declares and the
library exports the three _s calls, the two macros and the two side structures, the old layouts and the version are unchanged; the
refusals that need no device; and, on the reference side alone (tests/rdo_skip_ref.py), the conditions that keep the GPU sweep of
tests/test_gpu_rdo_skip.py from passing vacuously and the reference's own consistency, for every mode, clamped and not."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from flashgmm_amd import _lib
from tests import rdcurve_ref as V
from tests import rdo_skip_ref as S
from tests import rdo_weights_ref as W
from tests import rdoq_ref as Q
from tests import synth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["polya", "as", "logistic"]
LAM = 0.5


def test_header_declares_and_library_exports_the_calls():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"#define FGMM_HAS_RDO_SKIP 1\b", header) and re.search(r"#define FGMM_SKIP_VMAX 15\b", header) and "3f." in header
    assert re.search(r"typedef struct \{\s*int64_t \*skipped;[^}]*int64_t n_skipped;[^}]*int64_t n_eligible;[^}]*uint64_t ddist_q;[^}]*\} fgmm_rdo_skip;", header)
    assert re.search(r"typedef struct \{\s*uint64_t n_skipped\[FGMM_RDCURVE_MAX\];[^}]*int64_t n_eligible;[^}]*\} fgmm_rdcurve_skip;", header)
    for name, tail in (("fgmm_gmc_rdoq_batch_s", r"double lambda,\s*const fgmm_rdo_weights \*w[^,]*,\s*fgmm_rdo_skip \*skip"),
                       ("fgmm_gmc_rdcurve_batch_s", r"int n_lambda, const fgmm_rdo_weights \*w[^,]*,\s*fgmm_rdcurve_skip \*skip"),
                       ("fgmm_gmc_rdoq_budget_batch_s", r"fgmm_budget_result \*results[^,]*, const fgmm_rdo_weights \*w[^,]*,\s*fgmm_rdo_skip \*skip")):
        assert re.search(r"int\s+" + name + r"\s*\([^;]*" + tail + r"[^;]*\)\s*;", header), name
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name
    assert re.search(r"#define FGMM_ABI_VERSION\s+6\b", header)  # (not bumped: nothing existing changed)
    # the old layouts are what they were (tests/test_rdo_weights_cpu.py pins the same three figures)
    assert C.sizeof(_lib.fgmm_rdoq_item) == 128 and C.sizeof(_lib.fgmm_rdcurve_item) == 72 + 8 + 3 * 16 * 8 + 8 + 8 and C.sizeof(_lib.fgmm_budget_result) == 24
    assert C.sizeof(_lib.fgmm_rdo_skip) == 32 and C.sizeof(_lib.fgmm_rdcurve_skip) == 16 * 8 + 8
    assert [n for n, _ in _lib.fgmm_rdo_skip._fields_] == ["skipped", "n_skipped", "n_eligible", "ddist_q"]
    assert [n for n, _ in _lib.fgmm_rdcurve_skip._fields_] == ["n_skipped", "n_eligible"]
    # the _w signatures have not moved; the _s forms take one more pointer
    for name, n in (("fgmm_gmc_rdoq_batch", 8), ("fgmm_gmc_rdcurve_batch", 9), ("fgmm_gmc_rdoq_budget_batch", 13)):
        assert len(_lib.SIGNATURES[name + "_w"][1]) == n and len(_lib.SIGNATURES[name + "_s"][1]) == n + 1, name


def test_invalid_arguments_are_refused_before_any_device_is_touched():
    L = _lib.lib()
    w, sk, ck = (_lib.fgmm_rdo_weights * 1)(), (_lib.fgmm_rdo_skip * 1)(), (_lib.fgmm_rdcurve_skip * 1)()
    assert L.fgmm_gmc_rdoq_batch_w(None, None, None, 0, 0, 1, -1.0, w) == 1
    want = L.fgmm_last_error()
    assert L.fgmm_gmc_rdoq_batch_s(None, None, None, 0, 0, 1, -1.0, w, sk) == 1 and L.fgmm_last_error() == want and b"lambda" in want
    assert L.fgmm_gmc_rdcurve_batch_s(None, None, None, 0, 0, 1, (C.c_double * 1)(0.5), 17, w, ck) == 1 and b"n_lambda" in L.fgmm_last_error()
    assert L.fgmm_gmc_rdoq_budget_batch_s(None, None, None, 0, 0, 1, None, 0, None, 16.0, 9, None, w, sk) == 1 and b"refine" in L.fgmm_last_error()


def test_python_surface():
    import flashgmm_amd
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    gmc = flashgmm_amd.GaussianMixtureConditional(K=4)
    for name in ("quantize_rdo", "quantize_rdo_batch", "rd_curve", "rd_curve_batch", "quantize_to_budget", "quantize_to_budget_batch"):
        p = inspect.signature(getattr(gmc, name)).parameters["channel_skip"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, name
    q = flashgmm_amd.RdoQuantized(None, 0, 0, 0, 1, None)
    assert (q.n_skipped, q.n_eligible, q.skipped) == (None, None, None)
    b = flashgmm_amd.BudgetQuantized(None, 0, 0, 0, 1, None)
    assert isinstance(b, flashgmm_amd.RdoQuantized) and (b.n_skipped, b.n_eligible, b.skipped) == (None, None, None)
    c = flashgmm_amd.RdCurve([0.5], 0, [0], [0], [0])
    assert c.n_skipped is None and c.n_eligible is None
    assert GaussianMixtureConditionalLatentCodec().rdo_channel_skip is False and CheckerboardLatentCodec().rdo_channel_skip is False
    assert GaussianMixtureConditionalLatentCodec(rdo_lambda=0.5, rdo_channel_skip=True).rdo_channel_skip is True
    assert CheckerboardLatentCodec(rdo_lambda=0.5, rdo_channel_skip=True).rdo_channel_skip is True


def cases(clamp):
    return [(shape, seed, T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf)) for shape in Q.SHAPES for seed, zf in Q.SEEDS]


def weightings(shape):
    M, hw = shape[0], shape[1] * shape[2]
    return {"unit": (None, None), "fixed": (W.chan_w(M), W.pos_w(hw))}


@pytest.fixture(scope="module")
def priced(oracle):
    """the GPU sweep's cases priced once: {(mode, clamp, shape, seed): (case, priced)}"""
    L = _lib.lib()
    return {(mode, clamp, shape, seed): (case, V.price(oracle, L, mode, *case, clamp=clamp))
            for mode in MODES for clamp in (True, False) for shape, seed, case in cases(clamp)}


def test_the_sweep_skips_keeps_and_meets_the_symbol_bound(oracle, priced):
    """the non-vacuity conditions of the GPU sweep, at lambda = 0.5, unweighted and with the fixed test weights, in EVERY case: at least
    one channel is skipped and at least one eligible coded channel is kept; over the whole sweep at least one coded channel is
    ineligible through |v0| > 15"""
    n_vmax = 0
    for key, (case, p) in priced.items():
        mode, clamp, shape, seed = key
        hw = shape[1] * shape[2]
        for name, (cw, pw) in weightings(shape).items():
            ch = S.channels(p, LAM, W.weights_of(*case, cw, pw, clamp=clamp), hw)
            kept = int((~ch["skip"] & ~ch["inelig"]).sum())
            print(key, name, "coded", len(ch["skip"]), "skipped", int(ch["skip"].sum()), "eligible kept", kept, "over 15", int(ch["vmax"].sum()))
            assert ch["skip"].any(), (key, name)
            assert kept >= 1, (key, name)
            assert np.all(ch["nz0"] >= 1)
            n_vmax += int(ch["vmax"].sum())
    assert n_vmax >= 1


def test_lambda_zero_skips_nothing_and_the_result_reprices_to_its_own_sums(oracle, priced):
    L = _lib.lib()
    for key, (case, p) in priced.items():
        mode, clamp, shape, seed = key
        for name, (cw, pw) in weightings(shape).items():
            r0 = S.rdoq(oracle, L, mode, *case, 0.0, clamp=clamp, cw=cw, pw=pw, priced=p)
            b0 = W.rdoq(oracle, L, mode, *case, 0.0, clamp=clamp, cw=cw, pw=pw, priced=p)
            assert r0["n_skipped"] == 0 and not r0["skipped"].any() and r0["n_changed"] == 0 and r0["ddist_q"] == 0, (key, name)
            assert Q.same_float_bits(r0["y"], b0["y"]) and r0["bits_q_after"] == r0["bits_q_before"] == b0["bits_q_after"]
            for lam in (LAM, 5.0):
                r = S.rdoq(oracle, L, mode, *case, lam, clamp=clamp, cw=cw, pw=pw, priced=p)
                b = W.rdoq(oracle, L, mode, *case, lam, clamp=clamp, cw=cw, pw=pw, priced=p)
                # re-pricing y_rdo as a latent of its own: exactly bits_q_after, over exactly the channels of zero_bitmap
                again = V.curve(V.price(oracle, L, mode, r["y"], *case[1:], clamp=clamp), [0.0])
                assert again["bits_q_before"] == r["bits_q_after"] == int(r["chan_after"].sum()), (key, name, lam)
                assert r["zero_bitmap"] == T.to_coder_inputs(r["y"], *case[1:], clamp=clamp)[5].tolist()
                assert [int(v) for v in r["zero_bitmap"]] == [int(c > 0) for c in r["chan_after"]], (key, name, lam)
                # against the plain call: never more bits, the skipped channels' planes zero, the others untouched
                assert r["bits_q_after"] <= b["bits_q_after"] and r["bits_q_before"] == b["bits_q_before"]
                assert not r["y"][0, r["skipped"]].any() and Q.same_float_bits(r["y"][0, ~r["skipped"]], b["y"][0, ~r["skipped"]])
                assert r["n_skipped"] == int(r["skipped"].sum()) <= r["n_eligible"] <= len(r["coded"])


def test_the_skip_form_f_lies_below_the_plain_one_and_so_does_its_lambda(oracle, priced):
    L = _lib.lib()
    grid = [0.0] + [16.0 * 2.0 ** (j - 15) for j in range(1, 16)]
    for mode in MODES:
        for clamp in (True, False):
            for (shape, (seed, zf)), case in zip(V.BUDGET_CASES, V.budget_cases(clamp)):
                hw = shape[1] * shape[2]
                p = priced[mode, clamp, shape, seed][1] if (mode, clamp, shape, seed) in priced else V.price(oracle, L, mode, *case, clamp=clamp)
                for name, (cw, pw) in weightings(shape).items():
                    wt = W.weights_of(*case, cw, pw, clamp=clamp)
                    f_plain, f_skip = W.group_f(L, [p], [wt]), S.group_f(L, [p], [wt], [hw])
                    a, b = f_plain(grid), f_skip(grid)
                    assert all(y <= x for x, y in zip(a, b)), (mode, clamp, shape, seed, name)
                    budget = V.budget_of(a[0], f_plain([16.0])[0])
                    plain, skip = V.search(f_plain, budget), V.search(f_skip, budget)
                    assert skip["lam"] <= plain["lam"] and skip["status"] == 0 and skip["bytes_pred"] <= budget, (mode, clamp, shape, seed, name)
