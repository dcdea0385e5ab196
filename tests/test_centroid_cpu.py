"""CPU (-m "not gpu"): centroid reconstruction (include/flashgmm_amd.h section 3i) as far as it can be checked without a GPU - the header,
the library's export and the ctypes declaration; the float64 closed form of tests/centroid_ref.py against a quadrature of the mixture
density; the binary32 restatement of the header's sequence against that closed form, region by region; the wide form's series against it;
what the GPU tests rely on in the corpus; the benefit on latents drawn from their own mixtures; the refusals that need no device; the
Python surface.

No figure here comes from a run of the code under test: every bound is the condition of the sum (centroid_ref.allowance), the first term
the series leaves out, or the resolution of binary64."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec
from tests import centroid_ref as Z
from tests import like_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fgmm_gmc_centroid_batch"


def flat(t):
    return t.reshape(-1).numpy()


@pytest.fixture(scope="module")
def corpus():
    """computed once, left unchanged: the likelihood corpus, its float64 closed form and the binary32 restatement on the CPU"""
    t = [torch.from_numpy(a) for a in R.corpus()[:4]]
    return dict(t=t, c64=Z.centroid(*t, dtype=torch.float64, form="closed"), c32=Z.centroid(*t))


def test_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_HAS_CENTROID 1\b", header, re.M) and " 3i. " in header
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M) and _lib.lib().fgmm_abi_version() == 6  # no bump, as 3b - 3h
    assert NAME in header and hasattr(C.CDLL(_lib.LIB_PATH), NAME)
    res, args = _lib.SIGNATURES[NAME]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.POINTER(_lib.fgmm_centroid_item), C.c_int, C.c_float, C.c_float]
    # the struct begins with the fields fgmm_like_item begins with (check_latent_items serves it), then rec, n_kept, status
    it, like = _lib.fgmm_centroid_item, _lib.fgmm_like_item
    for name in ("y", "params", "M", "K", "hw"):
        assert getattr(it, name).offset == getattr(like, name).offset and getattr(it, name).size == getattr(like, name).size, name
    assert [(n, getattr(it, n).offset) for n, _ in it._fields_] == [("y", 0), ("params", 8), ("M", 56), ("K", 60), ("hw", 64), ("rec", 72), ("n_kept", 80),
                                                                    ("status", 88), ("pad_", 92)]
    assert C.sizeof(it) == 96 and _lib.CENTROID_ITEM_DTYPE.itemsize == 96
    body = re.search(r"typedef struct \{([^}]*)\} fgmm_centroid_item;", header).group(1)
    assert re.findall(r"(\w+)(?:, (\w+))?;", re.sub(r"/\*.*?\*/", "", body)) ==[("y", ""), ("params", ""), ("M", "K"), ("hw", ""), ("rec", ""), ("n_kept", ""), ("status", "pad_")]
    # the kernel and the call are files of their own, in the build and out of the fake-device build
    sh = open(os.path.join(ROOT, "flashgmm_amd", "csrc", "build.sh")).read()
    assert "fgmm_centroid.hip" in sh and "fgmm_centroid.cpp" in sh
    assert "fgmm_centroid" not in open(os.path.join(ROOT, "scripts", "tsan_host.sh")).read()


def test_closed_form_equals_a_quadrature_of_the_density(corpus):
    """about 100 rows of region (a) with every sigma > 0.3, kept ones: the closed form against composite Simpson on 20 001 nodes of the
    mixture density.  Simpson's own error, (b - a) step^4 max|g''''| / 180 with step 5e-5, is below 1e-15 here.  The closed form's is
    binary64 rounding of u and l (absolute 2^-53 each, as they are at most 1) carried through p = u - l into a * p / L: bounded by
    64 * 2^-53 * (1 + max_k a_k) / L per row."""
    y, sg, mu, pi = R.corpus()[:4]
    c64 = corpus["c64"]
    lo, hi = R.REGIONS["a"]
    ok = (sg.reshape(4, -1)[:, lo:hi] > 0.3).all(0) & flat(c64["keep"])[lo:hi]
    rows = (lo + np.flatnonzero(ok))[:100]
    assert len(rows) >= 80
    off_q, like_q = Z.quadrature(y, sg, mu, pi, rows)
    L = flat(c64["L"])[rows]
    bound = 64 * 2.0 ** -53 * (1.0 + c64["a"].reshape(4, -1).numpy()[:, rows].max(0)) / L + 1e-12
    err = np.abs(flat(c64["off"])[rows] - off_q)
    print(f"closed form against quadrature: max |off - off_q| {err.max():.3e}, largest bound {bound.max():.3e}, max |L - L_q| / L {np.abs(L - like_q).max() / L.min():.3e}")
    assert np.all(err <= bound) and np.all(np.abs(L - like_q) <= 64 * 2.0 ** -53 + 1e-12 * L)
    assert np.abs(off_q).max() > 0.05  # (the rows are not all centred bins)


def test_binary32_restatement_against_float64_per_region(corpus):
    """the header's binary32 sequence in torch against the float64 closed form, on the rows both keep and that are not ``near``: per row
    within centroid_ref.allowance - the condition of the sum at 8 ulps per library value.  Printed per region before it is asserted.
    The closed form evaluated in binary32 on every component (no series) is shown beside it: it leaves the allowance on the wide
    regions, which is why section 3i switches."""
    c64, c32 = corpus["c64"], corpus["c32"]
    lit = Z.centroid(*corpus["t"], form="closed")
    allow = flat(Z.allowance(Z.centroid(*corpus["t"], dtype=torch.float64)))
    rows = flat(c64["keep"]) & flat(c32["keep"]) & ~Z.near(flat(c64["L"]), flat(c64["off"]))
    err = np.abs(flat(c32["off"]).astype(np.float64) - flat(c64["off"]))
    err_lit = np.abs(flat(lit["off"]).astype(np.float64) - flat(c64["off"]))
    worst_literal = {}
    for name, (lo, hi) in R.REGIONS.items():
        r = rows[lo:hi]
        if not r.any():
            continue
        worst_literal[name] = float(np.nanmax(err_lit[lo:hi][flat(c64["keep"])[lo:hi]]))
        print(f"region ({name}): {int(r.sum()):3d} rows  max |off32 - off64| {err[lo:hi][r].max():.3e}  largest allowance {allow[lo:hi][r].max():.3e}  "
              f"(literal form in binary32: {worst_literal[name]:.3e})")
        assert np.all(err[lo:hi][r] <= allow[lo:hi][r]), name
    assert worst_literal["f"] > 1e-3 and worst_literal["e"] > 1e-2  # the literal form fails where components are wide


def test_series_against_the_closed_form_in_float64():
    """single components, sigma in [2, 3000] (some exactly 2, where the series is at its worst), a / sigma <= 4.5, in binary64: the
    three-term series is within centroid_ref.series_remainder - the first term it leaves out plus a bound of the rest - plus the closed
    form's own rounding, 64 * 2^-53 of its two cancelling terms.  In units of off = m / p."""
    rng = np.random.default_rng(R.SEED + 3)
    n = 4096
    sigma = np.exp(rng.uniform(np.log(2.0), np.log(3000.0), n))
    sigma[:8] = 2.0
    a = rng.uniform(0, 4.5, n) * sigma
    y = np.round(rng.standard_normal(n) * 4)
    sg = np.tile(sigma[None], (4, 1)).reshape(1, 4, n, 1).astype(np.float32)
    mu = np.tile((y - a)[None], (4, 1)).reshape(1, 4, n, 1).astype(np.float32)
    pi = np.zeros((1, 4, n, 1), np.float32)
    pi[:, 0] = 1.0
    t = [torch.from_numpy(x) for x in (y.reshape(1, 1, n, 1).astype(np.float32), sg, mu, pi)]
    closed, series = Z.centroid(*t, dtype=torch.float64, form="closed"), Z.centroid(*t, dtype=torch.float64, form="series")
    p = closed["p"][:, 0]
    bound = (Z.series_remainder(series)[:, 0] +64 * 2.0 ** -53 * (closed["a"] * closed["u_plus_l"] + closed["s"] * closed["f_plus"])[:, 0]) / p
    err = torch.abs(closed["off"] - series["off"])
    print(f"series against closed form: max |off| difference {float(err.max()):.3e}, largest bound {float(bound.max()):.3e}")
    assert bool(torch.all(err <= bound)) and float(bound.max()) < 1e-4 and float(torch.abs(closed["off"]).max()) > 0.05


def test_corpus_has_what_the_gpu_tests_rely_on(corpus):
    c64 = corpus["c64"]
    keep, wide = flat(c64["keep"]), c64["is_wide"].reshape(4, -1).numpy()
    share = {name: float(keep[lo:hi].mean()) for name, (lo, hi) in R.REGIONS.items()}
    print("kept share per region:", {k: round(v, 3) for k, v in share.items()})
    assert share["c"] == 0.0  # deep tail: L far below p_min
    assert 0.0 < share["e"] < 1.0 and 0.0 < share["g"] < 1.0  # |off| > 1/2 (wide, far means), negative weights: some kept, some dropped
    assert all(share[name] >= 0.99 for name in "abdf")
    for name in "ag":  # both forms of m_k occur
        lo, hi = R.REGIONS[name]
        assert wide[:, lo:hi].any() and not wide[:, lo:hi].all(), name
    # rows two precisions may decide differently: at most 1 % (none today); and the binary32 restatement decides as float64 elsewhere
    nr = Z.near(flat(c64["L"]), flat(c64["off"]))
    assert nr.mean() <= 0.01 and nr.sum() == 0
    assert np.array_equal(flat(corpus["c32"]["keep"])[~nr], keep[~nr])
    assert np.array_equal(flat(corpus["c32"]["rec"])[~keep], np.round(R.corpus()[0]).reshape(-1)[~keep])  # dropped rows: rec is v


def test_centroid_lowers_the_squared_error_on_sampled_latents():
    y, sg, mu, pi = Z.sample()
    assert y.shape == (1, 4, 32, 32)
    c64 = Z.centroid(*(torch.from_numpy(a) for a in (y, sg, mu, pi)), dtype=torch.float64, form="closed")
    e_round = float(np.mean((y.astype(np.float64) - np.round(y)) ** 2))
    e_rec = float(np.mean((y.astype(np.float64) - c64["rec"].numpy()) ** 2))
    print(f"mean squared latent error: rounding {e_round:.4f}, centroid {e_rec:.4f} ({100 * (e_rec / e_round - 1):+.0f} %), kept {float(c64['keep'].double().mean()):.3f}")
    assert e_rec < e_round
    assert abs(e_round - 1.0 / 12.0) < 0.01  # (the draws cover their bins: rounding sits at the uniform bin's 1/12)


def test_the_launch_form_cases_reach_all_16_forward_forms():
    """tests/test_gpu_centroid.py::test_every_launch_form runs the cases of tests/test_likelihood_logits_cpu.py: their FORWARD forms are
    every (positions per lane, plane type, grid) the launcher's ladder can pick for centroid_kernel"""
    from test_likelihood_logits_cpu import INSTANTIATION_CASES

    seen = {(R.FORMS[name, dt][0][0], dt, R.FORMS[name, dt][0][1]) for name, dt in INSTANTIATION_CASES}
    every = {(vec, dt, lin) for dt in R.ALL for lin in (True, False) for vec in ((1, 4) if dt == "f32" else (1, 4, 8))}
    assert len(every) == 16 and seen == every, sorted(every - seen)


def test_refusals_that_need_no_device():
    """a null context, a negative count and null items are refused before anything touches a device"""
    L = _lib.lib()
    arr = (_lib.fgmm_centroid_item * 1)()
    assert L.fgmm_gmc_centroid_batch(None, None, arr, 1, R.SB, Z.P_MIN) == 1
    assert b"bad argument" in L.fgmm_last_error()


def test_python_surface_fails_loudly_without_a_device():
    gmc = GaussianMixtureConditional(K=4)
    for name in ("reconstruct", "reconstruct_batch"):
        p = inspect.signature(getattr(GaussianMixtureConditional, name)).parameters
        assert list(p)[:5] == ["self", "y_hat" + ("s" if name.endswith("batch") else ""), "scales", "means", "weights"]
        for kw, default in (("weights_are_logits", False), ("p_min", 2.0 ** -16), ("return_kept", False)):
            assert p[kw].default == default and p[kw].kind is inspect.Parameter.KEYWORD_ONLY, (name, kw)
    y, sg, mu, pi = (torch.from_numpy(a) for a in R.corpus()[:4])
    with pytest.raises(RuntimeError, match="GPU only"):
        gmc.reconstruct(y, sg, mu, pi)
    with pytest.raises(RuntimeError, match="GPU only"):
        gmc.reconstruct_batch(y, sg, mu, pi)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            gmc.reconstruct(y, sg, mu, pi, p_min=bad)
        with pytest.raises(ValueError):
            GaussianMixtureConditionalLatentCodec(K=4, centroid=True, centroid_p_min=bad)
    with pytest.raises(RuntimeError):
        GaussianMixtureConditional(K=3).reconstruct(y, sg[:, :24], mu[:, :24], pi[:, :24])
    p = inspect.signature(GaussianMixtureConditionalLatentCodec.__init__).parameters
    assert p["centroid"].default is False and p["centroid_p_min"].default == 2.0 ** -16
    codec = GaussianMixtureConditionalLatentCodec(K=4)
    assert codec.centroid is False and GaussianMixtureConditionalLatentCodec(K=4, centroid=True, quantizer="weighted_mean_ste").centroid is True
    # the nine callables of the compiled boundary are what they were
    from flashgmm_amd import _boundary
    assert not any("centroid" in n or "reconstruct" in n for n in dir(_boundary))
