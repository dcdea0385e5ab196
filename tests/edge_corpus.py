"""The edge corpus shared by tests/test_reference_edges_cpu.py and tests/test_gpu_reference_edges.py: seeded generators of
the inputs where a GMM coder goes wrong, each family a named case so that a failure names its family.  Data only (numpy):
the expected answers are computed by the compiled reference (tests/ref_worker.py), never stored.

  PARAM_FAMILIES   (sigma, mu, pi) rows [n, 4] float32, plus symbols v and abscissae x1 < x2 for every row
  FP16_FAMILIES    the same as float16 planes (the device widens them; the reference is fed the widened floats)
  LATENT_FAMILIES  latents y [1, M, h, w] float32 with ordinary parameters: ties, -0.0, NaN / inf, |y| >= 2^31, and the values
                   that put abs_max at the limits of the coder's paths
  STREAM_FAMILIES  what a decoder is given instead of its bitstream: random bytes, truncations, a flipped word
  CLAMP_FAMILIES   rows (v, sigma, mu, pi) aimed at the guards of the clamped-sigma fast paths (flashgmm_amd/csrc/fgmm_math.h,
                   fgmm_tab.hip), each with a numpy predicate that restates its guard on the inputs (CLAMP_GUARDS)
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
I32_MIN, I32_MAX = -(2**31), 2**31 - 1


def _rng(name: str, seed: int = 0) -> np.random.Generator:
    return np.random.default_rng([seed, *name.encode()])


def _ordinary(rng, n):
    """KA-1-like rows: per-row scale e, sigma in [0.11, 2.1] e, mu ~ N(0, e), pi Dirichlet(1)"""
    e = np.exp(rng.uniform(-2, 2, n))[:, None]
    sg = (rng.uniform(0, 2, (n, 4)) + 0.11) * e
    mu = rng.standard_normal((n, 4)) * e
    pi = rng.dirichlet(np.ones(4), n)
    return sg.astype(F32), mu.astype(F32), pi.astype(F32)


def _spots(rng, n, frac=0.25):
    """(rows, components) of a random subset of the entries"""
    m = rng.random((n, 4)) < frac
    m[rng.integers(0, n, max(1, n // 8)), rng.integers(0, 4, max(1, n // 8))] = True
    return m


def _with(a, mask, vals):
    a = a.copy()
    a[mask] = np.resize(np.asarray(vals, F32), int(mask.sum()))
    return a


def _p_wide_sigma(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    return np.exp(rng.uniform(np.log(1e-5), np.log(3e3), (n, 4))).astype(F32), mu, pi


def _p_neg_sigma(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    m = _spots(rng, n)
    return _with(sg, m, -sg[m]), mu, pi


def _p_zero_sigma(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    return _with(sg, _spots(rng, n), [0.0, -0.0]), mu, pi


def _p_subnormal_sigma(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    sub = np.array([1e-45, 1e-40, 1.1754942e-38, -1e-42, 1.17549435e-38], F32)
    return _with(sg, _spots(rng, n), sub), mu, pi


def _p_nonfinite_sigma(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    return _with(sg, _spots(rng, n, 0.15), [np.inf, -np.inf, np.nan]), mu, pi


def _p_huge_mu(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    return sg, _with(mu, _spots(rng, n), [1e30, -1e30, 3e38, -3e38, 3.4028235e38]), pi


def _p_nonfinite_mu(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    return sg, _with(mu, _spots(rng, n, 0.15), [np.inf, -np.inf, np.nan]), pi


def _p_neg_weights(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    m = _spots(rng, n)
    return sg, mu, _with(pi, m, -pi[m] * F32(0.7))


def _p_weights_over_one(rng, n):
    """rows whose weights sum above 1 by one ulp .. 1e-4 (the largest component grows)"""
    sg, mu, pi = _ordinary(rng, n)
    pi = pi.copy()
    k = pi.argmax(1)
    ex = np.where(rng.random(n) < 0.5, np.spacing(F32(1)) * rng.integers(1, 4, n), rng.uniform(1e-7, 1e-4, n)).astype(F32)
    pi[np.arange(n), k] += ex
    return sg, mu, pi


def _p_nan_weights(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    return sg, mu, _with(pi, _spots(rng, n, 0.1), [np.nan, np.inf, -np.inf])


def _p_zero_weights(rng, n):
    sg, mu, pi = _ordinary(rng, n)
    pi = pi.copy()
    pi[rng.random(n) < 0.5] = 0.0
    return sg, mu, pi


def _p_tiny_and_huge_sigma(rng, n):
    """tiny and huge sigma in the same row"""
    sg, mu, pi = _ordinary(rng, n)
    sg = sg.copy()
    sg[:, 0] = np.exp(rng.uniform(np.log(1e-6), np.log(1e-2), n))
    sg[:, 3] = np.exp(rng.uniform(np.log(1e2), np.log(1e5), n))
    return sg, mu, pi


def _p_dip_weights(rng, n):
    """half the rows: 0.6 at -a, -0.3 at 0, 0.35 + 0.35 at +a - a CDF that rises, falls across several edges and rises to 1
    again: it decreases in the middle of its window only (monotone into both saturated tails)"""
    sg, mu, pi = _ordinary(rng, n)
    sg, mu, pi = sg.copy(), mu.copy(), pi.copy()
    d = rng.random(n) < 0.5
    a = rng.uniform(6, 12, n)
    mu[d] = np.stack([-a, rng.uniform(-1, 1, n), a, a + rng.uniform(0, 2, n)], 1)[d]
    sg[d] = np.stack([np.ones(n), rng.uniform(0.5, 1.5, n), np.ones(n), np.ones(n)], 1)[d]
    pi[d] = np.array([0.6, -0.3, 0.35, 0.35], F32)
    return sg, mu, pi


PARAM_FAMILIES = {
    "wide_sigma": _p_wide_sigma,
    "neg_sigma": _p_neg_sigma,
    "zero_sigma": _p_zero_sigma,
    "subnormal_sigma": _p_subnormal_sigma,
    "nonfinite_sigma": _p_nonfinite_sigma,
    "huge_mu": _p_huge_mu,
    "nonfinite_mu": _p_nonfinite_mu,
    "neg_weights": _p_neg_weights,
    "weights_over_one": _p_weights_over_one,
    "nan_weights": _p_nan_weights,
    "zero_weights": _p_zero_weights,
    "tiny_and_huge_sigma": _p_tiny_and_huge_sigma,
    "dip_weights": _p_dip_weights,
}


def symbols_for(rng, mu, n):
    """symbols: mostly near the row's first mean (the coded range), some anywhere in int32 and at its ends"""
    near = np.clip(np.nan_to_num(mu[:, 0], nan=0.0, posinf=0.0, neginf=0.0), -40, 40)
    v = np.rint(near + rng.standard_normal(n) * 4).astype(np.int64)
    far = rng.random(n) < 0.1
    v[far] = rng.integers(I32_MIN, I32_MAX, int(far.sum()), endpoint=True)
    ends = rng.random(n) < 0.02
    v[ends] = rng.choice([I32_MIN, I32_MIN + 1, I32_MAX, -32768, 32767, 2**31 - 128, -(2**31) + 128], int(ends.sum()))
    return v.astype(np.int32)


def abscissae_for(rng, n):
    """arbitrary float abscissae x1 < x2 (any distance, far tails, the int32 ends)"""
    x1 = (rng.standard_normal(n) * np.exp(rng.uniform(-3, 25, n))).astype(F32)
    x2 = (x1 + np.exp(rng.uniform(-10, 10, n))).astype(F32)
    return x1, x2


def param_case(family: str, n: int = 4096, seed: int = 0):
    """-> dict(s, m, w [n, 4] float32; v int32 [n]; x1, x2 float32 [n])"""
    rng = _rng(family, seed)
    s, m, w = PARAM_FAMILIES[family](rng, n)
    v = symbols_for(rng, m, n)
    x1, x2 = abscissae_for(rng, n)
    return {"s": np.ascontiguousarray(s, F32), "m": np.ascontiguousarray(m, F32), "w": np.ascontiguousarray(w, F32),
            "v": v, "x1": x1, "x2": x2}


def param_case_after(family: str, n: int, n_head: int, seed: int = 0):
    """param_case whose first n_head rows are ordinary ones: the family's rows only from n_head on (a checkpointed stream's
    last segment holds them alone, so no note downstream of them can catch a wrong symbol there)"""
    c = param_case(family, n, seed)
    s, m, w = _ordinary(_rng(family + "/head", seed), n_head)
    c["s"][:n_head], c["m"][:n_head], c["w"][:n_head] = s, m, w
    return c


# ---- fp16 planes ------------------------------------------------------------------------------------------------------
def _h_subnormal(rng, n):
    s, m, w = _ordinary(rng, n)
    s16, m16, w16 = s.astype(np.float16), m.astype(np.float16), w.astype(np.float16)
    sub = np.array([6e-8, 1e-6, 3e-5, 6.1e-5], np.float16)  # the subnormal halves (the smallest normal one is 6.104e-5)
    mk = _spots(rng, n)
    s16[mk] = np.resize(sub, int(mk.sum()))
    mk = _spots(rng, n)
    m16[mk] = np.resize(-sub, int(mk.sum()))
    return s16, m16, w16


def _h_max(rng, n):
    s, m, w = _ordinary(rng, n)
    s16, m16, w16 = s.astype(np.float16), m.astype(np.float16), w.astype(np.float16)
    mk = _spots(rng, n)
    m16[mk] = np.resize(np.array([65504, -65504], np.float16), int(mk.sum()))
    sk = _spots(rng, n, 0.1)
    s16[sk] = np.float16(65504)
    return s16, m16, w16


def _h_inf(rng, n):
    s, m, w = _ordinary(rng, n)
    s16, m16, w16 = s.astype(np.float16), m.astype(np.float16), w.astype(np.float16)
    for a in (s16, m16):
        mk = _spots(rng, n, 0.08)
        a[mk] = np.resize(np.array([np.inf, -np.inf], np.float16), int(mk.sum()))
    return s16, m16, w16


def _h_weights_nearest(rng, n):
    """weights rounded to NEAREST (tests/synth.py's helper rounds toward zero): some rows sum above 1"""
    s, m, w = _ordinary(rng, n)
    return s.astype(np.float16), m.astype(np.float16), w.astype(np.float16)


FP16_FAMILIES = {
    "f16_subnormal": _h_subnormal,
    "f16_max": _h_max,
    "f16_inf": _h_inf,
    "f16_weights_nearest": _h_weights_nearest,
}


def fp16_case(family: str, M: int = 8, h: int = 8, w: int = 12, seed: int = 0):
    """-> (y [1, M, h, w] float32, sigma, mu, pi planes [1, 4M, h, w] float16)"""
    rng = _rng(family, seed)
    n = M * h * w
    s16, m16, w16 = FP16_FAMILIES[family](rng, n)
    e = np.exp(rng.uniform(-1, 1.5, M)).astype(F32)
    y = (rng.standard_normal((1, M, h, w)) * 1.5 * e[None, :, None, None]).astype(F32)

    def planes(a):  # rows are (channel, position) in order, component k -> channel k*M + c
        return np.ascontiguousarray(a.reshape(M, h, w, 4).transpose(3, 0, 1, 2).reshape(1, 4 * M, h, w))

    return y, planes(s16), planes(m16), planes(w16)


# ---- latents -----------------------------------------------------------------------------------------------------------
def _l_base(rng, M, h, w):
    e = np.exp(rng.uniform(-1, 1.5, M)).astype(F32)
    return (rng.standard_normal((1, M, h, w)) * 1.5 * e[None, :, None, None]).astype(F32)


def _put(y, rng, vals):
    """the values at distinct random places of y (in place)"""
    flat = y.reshape(-1)
    at = rng.choice(flat.size, len(vals), replace=False)
    flat[at] = np.asarray(vals, F32)
    return y


def _l_ties(rng, M, h, w):
    y = _l_base(rng, M, h, w)
    k = rng.integers(-6, 6, y.size)
    half = rng.random(y.size) < 0.5
    y.reshape(-1)[half] = (k[half] + 0.5).astype(F32)
    return y


def _l_neg_zero(rng, M, h, w):
    y = _l_base(rng, M, h, w)
    y[0, 1] = -0.0
    y[0, 2] = np.where(rng.random((h, w)) < 0.5, F32(-0.0), F32(-0.4))
    return _put(y, rng, [-0.0] * 7)


def _l_all_negative(rng, M, h, w):
    return -np.abs(_l_base(rng, M, h, w)) - F32(0.6)


def _l_one_nan(rng, M, h, w):
    return _put(_l_base(rng, M, h, w), rng, [np.nan])


def _l_one_posinf(rng, M, h, w):
    return _put(_l_base(rng, M, h, w), rng, [np.inf])


def _l_one_neginf(rng, M, h, w):
    return _put(_l_base(rng, M, h, w), rng, [-np.inf])


def _l_beyond_int32(rng, M, h, w):
    return _put(_l_base(rng, M, h, w), rng, [2147483648.0, -2147483904.0, 3e9, -5e12, 1e38])


def _l_beyond_int32_mean_there(rng, M, h, w):
    return _put(_l_base(rng, M, h, w), rng, [np.nan, np.inf, -np.inf, 3e9, -2147483904.0, 2147483648.0])


def _l_near_int32_end(rng, M, h, w):
    """just below and above 2^31 - 128 (the last float below 2^31), and the int32 minimum"""
    return _put(_l_base(rng, M, h, w), rng, [2147483520.0, np.nextafter(F32(2147483520.0), F32(0)), -2147483520.0,
                                             -2147483648.0, 2147483392.0])


def _abs_max_at(am):
    def make(rng, M, h, w):
        y = np.clip(_l_base(rng, M, h, w), -(am - 1), am - 1)
        return _put(y, rng, [am - 1 + 0.25, -(am - 1) - 0.4])  # max(|trunc|) = am - 1 -> abs_max = am
    return make


LATENT_FAMILIES = {
    "ties_half": _l_ties,
    "neg_zero": _l_neg_zero,
    "all_negative": _l_all_negative,
    "one_nan": _l_one_nan,
    "one_posinf": _l_one_posinf,
    "one_neginf": _l_one_neginf,
    "beyond_int32": _l_beyond_int32,
    "beyond_int32_mean_there": _l_beyond_int32_mean_there,  # (latent_case puts means at -2^31 and at the latent itself)
    "near_int32_end": _l_near_int32_end,
    "abs_max_32767": _abs_max_at(32767),
    "abs_max_32768": _abs_max_at(32768),
    "hdr2_max_bs_126": _abs_max_at(125),     # abs_max + 1 = 126: 2-byte headers (tests/helpers.py:hdr_form)
    "hdr4_max_bs_127": _abs_max_at(126),     # 127: 4-byte headers
    "hdr4_max_bs_16382": _abs_max_at(16381),  # MAX_BS_H4: the last 4-byte form
    "hdr8_max_bs_16383": _abs_max_at(16382),
    "segdec_am_1022": _abs_max_at(1022),     # 2 * (am + 1) + 2 = 2048: the GPU segment decoder's last width
    "segdec_am_1023": _abs_max_at(1023),     # 2050: beyond it
}
# the segment decoder takes checkpointed items only: these families are drawn with LATENT_SHAPE (seven notes at stride 256
# per channel group of 512 latents), the others with latent_case's default shape
LATENT_SHAPE = {"segdec_am_1022": (12, 16, 32), "segdec_am_1023": (12, 16, 32)}


def latent_case(family: str, M: int = 12, h: int = 8, w: int = 16, seed: int = 0):
    """-> (y [1, M, h, w], sigma, mu, pi [1, 4M, h, w]) float32, ordinary parameters (sigma scaled with the channel's latents).
    (M, h, w) is LATENT_SHAPE's where the family has one there."""
    M, h, w = LATENT_SHAPE.get(family, (M, h, w))
    rng = _rng(family, seed)
    y = LATENT_FAMILIES[family](rng, M, h, w)
    n = M * h * w
    s, m, p = _ordinary(rng, n)
    if family == "beyond_int32_mean_there":  # a mixture centred where the out-of-range latent's symbol INT32_MIN lies, and
        far = ~(np.abs(y.reshape(-1)) < 2**31)  # one at the latent itself (finite ones): both edges are still the same float
        m[far, 0] = F32(-2147483648.0)
        m[far, 1] = np.where(np.isfinite(y.reshape(-1)[far]), y.reshape(-1)[far], F32(0))
        s[far, :2] = F32(1.0)

    def planes(a):
        return np.ascontiguousarray(a.reshape(M, h, w, 4).transpose(3, 0, 1, 2).reshape(1, 4 * M, h, w))

    return np.ascontiguousarray(y, F32), planes(s), planes(m), planes(p)


# ---- the clamped-sigma fast paths ------------------------------------------------------------------------------------------
# With clamp_scales=True (every real caller) the kernels run packed-fp32 fast sequences behind guards and hand back to the IEEE
# sequence outside them.  Every family below is a function of (rng, n) -> (v int32 [n], sigma, mu, pi [n, 4] float32): rows that
# lie on both sides of one guard, the constants taken from the line that holds the guard.  |v| stays small enough for every
# decoder (abs_max + 1 far below 40000), and sigma is given PRE-clamp.
GUARD_A = 2048.0                      # fgmm_math.h mix4_clamped2: `fabsf(a.x) < 0x1p11f`, a.x = (v - 0.5) - mu_k
RCP_TAME = 2.0**60                    # fgmm_math.h tame(): `fabsf(a) < 0x1p60f`, Phi2<MODE_LOGISTIC>'s per-half guard on d = 1 + e
LOGISTIC_C = F32(1.702)               # fgmm_math.h Phi<MODE_LOGISTIC>: e = exp(-1.0f * (1.702f * z))
EXP_HI = 88.3762626647949             # fgmm_math.h exp_ref: the upper clamp of the argument
SIGMA_LO, SIGMA_HI = F32(0.11), F32(256.0)  # fgmm_math.h clamp_scale / Sigma4::set (entropy_models.py:817)
SAT_Z = {"polya": (5.25, 5.0), "as": (5.45, 5.45), "logistic": (8.2, 9.8)}  # fgmm_math.h Sat<MODE>::ZL, ZR
SEGDEC_AM = 1022                      # fgmm_decode_gpu.cpp: the segment decoder takes 2 * (abs_max + 1) + 2 <= 2048
# the distances mix4_clamped2's compare is probed at (both signs); beyond the issue's list a few far ones below 2^40, where
# exp_nonpos2's un-clamped argument (valid to -2^30) would leave its domain if the compare let them through
GUARD_BELOW = (2047.0, 2047.5, float(np.nextafter(F32(2048), F32(0))))
GUARD_ABOVE = (2048.0, float(np.nextafter(F32(2048), F32(4096))), 2048.5, 2049.0, 4096.0, 2.0**16, 2.0**24, 2.0**32, 2.0**39)


def clamp_sigma(s):
    """torch.clamp(s, 0.11, 256) on float32: NaN kept, -0 / negative / -inf -> 0.11, +inf -> 256"""
    with np.errstate(invalid="ignore"):
        return np.clip(np.asarray(s, F32), SIGMA_LO, SIGMA_HI)


def _near_symbols(rng, n, lim=40):
    return rng.integers(-lim, lim, n, endpoint=True).astype(np.int32)


def _ordinary_at(rng, v):
    """ordinary rows whose means lie near the row's symbol"""
    n = len(v)
    sg, mu, pi = _ordinary(rng, n)
    return sg, (mu + v[:, None].astype(F32)).astype(F32), pi


def _c_guard_2048(rng, n):
    """(v - 0.5) - mu_k exactly on +-GUARD_BELOW / +-GUARD_ABOVE in one, two or all four components (fgmm_math.h mix4_clamped2,
    the 0x1p11f compare).  The symbol's sign is chosen so that mu = x - a is a binary32 and x - mu gives a back exactly: for
    2048 - ulp the mean must stay below 2048 in magnitude (x and a of one sign), for 2048 + ulp above it (opposite signs)."""
    below = rng.random(n) < 0.45
    a = np.where(below, rng.choice(GUARD_BELOW, n), rng.choice(GUARD_ABOVE, n))
    sa = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    sx = np.where(a < 2048, sa, -sa)
    v = (sx * rng.integers(1, 40, n, endpoint=True)).astype(np.int32)
    sg, mu, pi = _ordinary_at(rng, v)
    x = v.astype(np.float64) - 0.5
    far = (x - sa * a).astype(F32)
    how = rng.integers(0, 3, n)  # one, two, all four components
    k0 = rng.integers(0, 4, n)
    hit = np.zeros((n, 4), bool)
    hit[np.arange(n), k0] = True
    hit[np.arange(n), (k0 + 1) % 4] |= how >= 1
    hit[how == 2] = True
    mu = np.where(hit, far[:, None], mu).astype(F32)
    # sigma of the far components: both ends of the clamp and beyond, so that z = a / sigma runs from 8 to 2^39 / 0.11
    sg = np.where(hit, rng.choice(np.array([0.05, 0.11, 1.0, 200.0, 256.0, 1000.0], F32), (n, 4)), sg).astype(F32)
    return v, sg, mu, pi


def _spread(rng, n, lim, lo0, hi0, gap_lo, gap_hi):
    """mu_0 in [lo0, hi0], mu_1 = mu_0 + [gap_lo, gap_hi] (more than 2^11 and less than 2^12 apart: some edges are within 2^11
    of all four means, others are not), mu_2, mu_3 between them; wide sigma so that the far components are not saturated
    everywhere; symbols anywhere in [-lim, lim]"""
    mu = np.empty((n, 4))
    mu[:, 0] = rng.uniform(lo0, hi0, n)
    mu[:, 1] = mu[:, 0] + rng.uniform(gap_lo, gap_hi, n)
    mu[:, 2:] = mu[:, :1] + rng.uniform(0, 1, (n, 2)) * (mu[:, 1:2] - mu[:, :1])
    sg = np.exp(rng.uniform(np.log(0.05), np.log(600.0), (n, 4)))
    sg[:, :2] = rng.uniform(60, 300, (n, 2))
    pi = rng.dirichlet(np.ones(4), n)
    near = mu[np.arange(n), rng.integers(0, 4, n)] + rng.standard_normal(n) * 30
    v = np.clip(np.rint(np.where(rng.random(n) < 0.5, near, rng.uniform(-lim, lim, n))), -lim, lim).astype(np.int32)
    v[:2] = (lim, -lim)
    return v, sg.astype(F32), mu.astype(F32), pi.astype(F32)


def _c_spread_means(rng, n):
    """means inside the coded range, abs_max of about three thousand (4-byte headers): fgmm_tab.hip tab_kernel phase 2 decides
    fast / slow per pair of edges, and a row's window spans both kinds"""
    return _spread(rng, n, 3000, -1900.0, -1100.0, 2100.0, 3900.0)


def _c_spread_means_1022(rng, n):
    """spread_means' second shape: abs_max <= SEGDEC_AM (the GPU segment decoder's width limit) with mu_0 and mu_1 OUTSIDE
    the coded range, about -1500 and +1500: |x - mu_k| still crosses 2^11 inside the row (fgmm_tab.hip segdec_kernel)"""
    return _spread(rng, n, SEGDEC_AM - 1, -1900.0, -1300.0, 2950.0, 3500.0)


def _c_spread_means_510(rng, n):
    """the same with abs_max <= 510: 2 * 511 + 2 = 1024 edges, the widest row the single-pass table kernel takes (fgmm_internal.h
    tab_tl: at least 16 latents per block of 16384 edges), so that tab_kernel's phase 2 sees mixed rows in a decode too"""
    return _spread(rng, n, 509, -1900.0, -1300.0, 2950.0, 3500.0)


def _c_nan_sigma_one(rng, n):
    """NaN in exactly one, two, three and four sigmas of half the rows, the others ordinary (fgmm_math.h Sigma4::set: `tame`)"""
    v = _near_symbols(rng, n)
    sg, mu, pi = _ordinary_at(rng, v)
    cnt = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 4, n, endpoint=True))
    order = np.argsort(rng.random((n, 4)), 1)
    sg = sg.copy()
    sg[np.argsort(order, 1) < cnt[:, None]] = np.nan
    return v, sg, mu, pi


SIGMA_AT_CLAMP = np.array([np.nextafter(SIGMA_LO, F32(0)), SIGMA_LO, np.nextafter(SIGMA_LO, F32(1)), np.nextafter(SIGMA_HI, F32(0)),
                           SIGMA_HI, np.nextafter(SIGMA_HI, F32(1e3)), 0.0, -0.0, 1e-40, -1.5, -np.inf, np.inf,
                           np.finfo(F32).max], F32)


def _c_sigma_at_clamp(rng, n):
    """sigma at, one ulp inside and one ulp outside both ends of the clamp, and the values only the clamp makes legal
    (fgmm_math.h Sigma4::set's v_med3_f32 against clamp_scale)"""
    v = _near_symbols(rng, n)
    sg, mu, pi = _ordinary_at(rng, v)
    m = _spots(rng, n, 0.3)
    m[rng.random(n) < 0.3] = False
    sg = sg.copy()
    sg[m] = rng.choice(SIGMA_AT_CLAMP, int(m.sum()))
    return v, sg, mu, pi


def _c_logistic_rcp_guard(rng, n):
    """z with 1 + exp(-1.702 z) just below, at and above 2^60 (fgmm_math.h Phi2<MODE_LOGISTIC>, tame(d.x) && tame(d.y)) in one or
    all four components: every binary32 within 64 ulp of the threshold z = -60 ln 2 / 1.702 (sigma 1: z = x - mu exactly), a
    band around it, and sigma 0.11 with x - mu down to -2047 (the exponential at its upper clamp)"""
    v = _near_symbols(rng, n, 8)
    sg, mu, pi = _ordinary_at(rng, v)
    x = v.astype(np.float64) - 0.5
    zt = F32(-60.0 * np.log(2.0) / 1.702)
    kind = rng.integers(0, 4, n)
    z = np.where(kind == 0, zt + rng.integers(-64, 64, n, endpoint=True) * np.spacing(zt),
                 np.where(kind == 1, rng.uniform(-60, -24.5, n), np.where(kind == 2, rng.uniform(-24.4, -10, n), 0.0)))
    s_hit = np.where(kind == 3, SIGMA_LO, F32(1.0)).astype(F32)
    a = np.where(kind == 3, np.where(rng.random(n) < 0.2, -2047.0, -np.exp(rng.uniform(np.log(1.0), np.log(2047.0), n))), z)
    hit = np.zeros((n, 4), bool)
    hit[np.arange(n), rng.integers(0, 4, n)] = True
    hit[rng.random(n) < 0.3] = True
    mu = np.where(hit, (x - a)[:, None], mu).astype(F32)
    sg = np.where(hit, s_hit[:, None], sg).astype(F32)
    return v, sg, mu, pi


def _c_sat_edges(rng, n):
    """(v - 0.5 - mu_k) / sigma_k within a few ulp of -ZL and +ZR of each mode at a v inside the range, for one component and for
    all four, sigma 0.11 and 256 among them (fgmm_decframe.h tab_window: the rounding of vL / vR and their - 1.0f / + 1.0f)"""
    v = _near_symbols(rng, n)
    sg, mu, pi = _ordinary_at(rng, v)
    zs = np.array([c for zl, zr in SAT_Z.values() for c in (-zl, zr)], F32)
    z = rng.choice(zs, n)
    s_hit = rng.choice(np.array([0.11, 0.25, 1.0, 3.0, 17.5, 256.0], F32), n)
    vt = rng.integers(-30, 30, n, endpoint=True)
    m_hit = ((vt - 0.5).astype(F32) - z * s_hit).astype(F32)  # z(vt) = (vt - 0.5 - mu) / sigma ~ z
    m_hit = (m_hit + rng.integers(-3, 3, n, endpoint=True) * np.spacing(m_hit)).astype(F32)
    hit = np.zeros((n, 4), bool)
    hit[np.arange(n), rng.integers(0, 4, n)] = True
    hit[rng.random(n) < 0.4] = True
    return v, np.where(hit, s_hit[:, None], sg).astype(F32), np.where(hit, m_hit[:, None], mu).astype(F32), pi


def _c_window_weights(rng, n):
    """weights for which tab_window must refuse the pruning lemma (fgmm_math.h Sat<MODE>::weight_ok) or T_sat = quant16(sum pi)
    is unusual (fgmm_decframe.h tab_window): 1 + ulp, -0.0, tiny negative, a sum above one whose quant16 wraps past 65535, a sum
    below one, all zero, one NaN, +inf, and a weight of tens to millions"""
    v = _near_symbols(rng, n)
    sg, mu, pi = _ordinary_at(rng, v)
    pi = pi.copy()
    kind = rng.integers(0, 12, n)
    k = rng.integers(0, 4, n)
    r = np.arange(n)
    one_hot = np.zeros((n, 4), F32)
    one_hot[r, k] = 1.0
    sel = kind == 0  # one weight of 1 + ulp, the others +0
    pi[sel] = one_hot[sel] * np.nextafter(F32(1), F32(2))
    sel = kind == 1  # -0.0 beside ordinary weights
    pi[r[sel], k[sel]] = -0.0
    sel = kind == 2  # tiny negative
    pi[r[sel], k[sel]] = rng.choice(np.array([-1e-45, -1e-30, -1e-8], F32), int(sel.sum()))
    sel = kind == 3  # a sum above one: (sum pi) * 65535 >= 65536 wraps in 16 bits
    pi[sel] = (pi[sel] * rng.uniform(1.1, 3.0, (int(sel.sum()), 1))).astype(F32)
    sel = kind == 4  # a sum below one
    pi[sel] = (pi[sel] * rng.uniform(0.05, 0.98, (int(sel.sum()), 1))).astype(F32)
    pi[kind == 5] = 0.0
    sel = (kind == 6) | (kind == 10)
    pi[r[sel], k[sel]] = np.nan
    sel = (kind == 7) | (kind == 11)
    pi[r[sel], k[sel]] = np.inf
    sel = kind == 8  # exactly one: a weight of 1.0f and three +0 (weight_ok's upper end, inside)
    pi[sel] = one_hot[sel]
    sel = kind == 9  # far outside [0, 1]: the logistic left tail's 2^-20 bound times such a weight is a whole count of the 16-bit CDF
    pi[r[sel], k[sel]] = rng.choice(np.array([20.0, 1000.0, 1e6, -50.0, -4000.0], F32), int(sel.sum()))
    return v, sg, mu, pi


CLAMP_FAMILIES = {
    "guard_2048": _c_guard_2048,
    "spread_means": _c_spread_means,
    "spread_means_1022": _c_spread_means_1022,
    "spread_means_510": _c_spread_means_510,
    "nan_sigma_one": _c_nan_sigma_one,
    "sigma_at_clamp": _c_sigma_at_clamp,
    "logistic_rcp_guard": _c_logistic_rcp_guard,
    "sat_edges": _c_sat_edges,
    "window_weights": _c_window_weights,
}
# Families that keep their character as float16 planes (rounded to nearest): NaN sigmas and the weights' NaN / inf / -0.0 / sums
# above one survive as they are; guard_2048's means near +-2048 round to even integers, so |x - mu| still lies on both sides of
# 2^11, no longer at the listed distances.  The others do not: 0.11 +- ulp, the 64-ulp band of logistic_rcp_guard and the few
# ulp of sat_edges collapse, and spread_means' sigma and means lose what separates its rows from wide_sigma's.
CLAMP_FP16_FAMILIES = ("guard_2048", "nan_sigma_one", "window_weights")
# Families whose rows can decrease under the clamp (negative, NaN or infinite weights): the ones the segment decoder must hand back
CLAMP_NONMONO_FAMILIES = ("neg_weights", "nan_weights", "dip_weights", "window_weights")


def clamp_case(family: str, n: int = 2304, seed: int = 0):
    """-> dict(v int32 [n]; s, m, w [n, 4] float32, sigma PRE-clamp) of a CLAMP_FAMILIES family"""
    v, s, m, w = CLAMP_FAMILIES[family](_rng("clamp/" + family, seed), n)
    return {"v": np.ascontiguousarray(v, np.int32), "s": np.ascontiguousarray(s, F32), "m": np.ascontiguousarray(m, F32),
            "w": np.ascontiguousarray(w, F32)}


def clamp_case_after(family: str, n: int, n_head: int, seed: int = 0):
    """a family of CLAMP_FAMILIES or PARAM_FAMILIES whose first n_head rows are ordinary ones (param_case_after's construction),
    symbols within +-40"""
    if family in CLAMP_FAMILIES:
        c = clamp_case(family, n, seed)
    else:
        c = {k: a for k, a in param_case(family, n, seed).items() if k in ("v", "s", "m", "w")}
        c["v"] = np.clip(c["v"], -40, 40).astype(np.int32)
    s, m, w = _ordinary(_rng(family + "/head", seed), n_head)
    c["s"][:n_head], c["m"][:n_head], c["w"][:n_head] = s, m, w
    c["v"][:n_head] = np.clip(c["v"][:n_head], -40, 40)
    return c


# ---- the guards, restated on the inputs: each -> bool [n], True where the row stays on the FAST side -----------------------
def _a_of(c):
    """(v - 0.5) - mu_k as the kernels compute it: binary32, one rounding"""
    x = (c["v"].astype(F32) - F32(0.5)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (x[:, None] - c["m"]).astype(F32)


def guard_tame_sigma(c):
    """Sigma4::set: no sigma is NaN"""
    return ~np.isnan(c["s"]).any(1)


def guard_near_means(c):
    """sym_entry's fast path: Sigma4::tame and every |(v - 0.5) - mu_k| < 2^11 (False for NaN / inf)"""
    with np.errstate(invalid="ignore"):
        return guard_tame_sigma(c) & (np.abs(_a_of(c)) < F32(GUARD_A)).all(1)


def guard_clamp_idle(c):
    """the clamp changes no sigma of the row"""
    with np.errstate(invalid="ignore"):
        return (clamp_sigma(c["s"]).view(np.uint32) == c["s"].view(np.uint32)).all(1)


def guard_logistic_rcp(c):
    """Phi2<MODE_LOGISTIC>: d = 1 + exp(-1.702 z) < 2^60 in both halves (x = v - 0.5 and x + 1) of every component.  z and the
    exponential's argument in binary32 as the kernel rounds them; the exponential itself in double (rows within the last ulp of
    the threshold may fall on either side here: the split that is asserted counts quarters)"""
    ok = np.ones(len(c["v"]), bool)
    s = clamp_sigma(c["s"])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for a in (_a_of(c), (_a_of(c) + F32(1)).astype(F32)):
            z = (a / s).astype(F32)
            arg = -(LOGISTIC_C * z).astype(F32)
            d = 1.0 + np.exp(np.minimum(arg.astype(np.float64), EXP_HI))
            ok &= (d < RCP_TAME).all(1)
    return ok


def guard_weights_logistic(c):
    """Sat<MODE_LOGISTIC>::weight_ok for all four: 0 <= pi <= 1 (-0.0 passes, NaN does not)"""
    with np.errstate(invalid="ignore"):
        return ((c["w"] >= 0) & (c["w"] <= 1)).all(1)


def guard_weights_finite(c):
    """Sat<MODE_POLYA / MODE_AS>::weight_ok for all four: finite"""
    return np.isfinite(c["w"]).all(1)


def near_sat_edge(c, max_bs: int, ulps: int = 8):
    """rows where some component's z at some edge v - 0.5, v in [-max_bs, max_bs + 1], lies within `ulps` of a -ZL or +ZR"""
    s = clamp_sigma(c["s"])
    hit = np.zeros(len(c["v"]), bool)
    x = (np.arange(-max_bs, max_bs + 2).astype(F32) - F32(0.5)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        z = ((x[None, :, None] - c["m"][:, None, :]) / s[:, None, :]).astype(F32)
        for zl, zr in SAT_Z.values():
            for t in (F32(-zl), F32(zr)):
                hit |= (np.abs(z - t) <= ulps * np.spacing(np.abs(t))).any((1, 2))
    return hit


def window_pair_kinds(c, max_bs: int):
    """-> (fast [n], slow [n]): the number of integer v in [-max_bs, max_bs] between the row's smallest and largest mean - edges
    every mode's evaluation window holds, since z changes sign there - whose edge v - 0.5 is within 2^11 of all four means, and
    the number where it is not"""
    vv = np.arange(-max_bs, max_bs + 1)
    x = (vv.astype(F32) - F32(0.5)).astype(F32)
    inside = (vv[None, :] >= np.ceil(c["m"].min(1))[:, None]) & (vv[None, :] <= np.floor(c["m"].max(1))[:, None])
    near = (np.abs((x[None, :, None] - c["m"][:, None, :]).astype(F32)) < F32(GUARD_A)).all(2)
    return (inside & near).sum(1), (inside & ~near).sum(1)


# family -> the guards it names: at least a quarter of its rows lie on each side of every one of them
CLAMP_GUARDS = {
    "guard_2048": (guard_near_means,),
    "nan_sigma_one": (guard_tame_sigma,),
    "sigma_at_clamp": (guard_clamp_idle,),
    "logistic_rcp_guard": (guard_logistic_rcp,),
    "window_weights": (guard_weights_logistic, guard_weights_finite),
}


# ---- streams -----------------------------------------------------------------------------------------------------------
STREAM_FAMILIES = ("random", "truncated", "flipped")


def stream_cases(family: str, valid: bytes, n: int, seed: int = 0, tail_from: int = 0):
    """-> [(tag, bytes)] of one family, derived from a valid stream for n symbols (lengths multiples of 4, >= 8).
    tail_from > 0 (a byte offset): "flipped" also corrupts only the words from there on - a checkpointed stream's last
    segment, which no note verifies"""
    rng = _rng(family, seed)
    if family == "random":
        return [(f"random{k}", rng.integers(0, 256, L, dtype=np.uint8).tobytes())
                for k, L in enumerate((8, 4 * (n // 4 + 8), 4 * (n + 64)))]
    if family == "truncated":  # every multiple of 4 in a short window below the full length, and a few far shorter
        L = len(valid)
        cuts = sorted({c for c in range(max(8, L - 40), L, 4)} | {8, max(8, (L // 8) * 4)})
        return [(f"cut{c}", valid[:c]) for c in cuts]
    assert family == "flipped"
    out = []
    for k in range(4):
        b = bytearray(valid)
        wi = int(rng.integers(0, len(valid) // 4))
        b[4 * wi: 4 * wi + 4] = (int.from_bytes(b[4 * wi: 4 * wi + 4], "little") ^ int(rng.integers(1, 2**32))).to_bytes(4, "little")
        out.append((f"flip{k}@{wi}", bytes(b)))
    if tail_from:
        for k in range(3):
            b = bytearray(valid)
            k0 = (tail_from + 4 * int(rng.integers(0, max(1, (len(valid) - tail_from) // 8)))) & ~3
            b[k0:] = rng.integers(0, 256, len(valid) - k0, dtype=np.uint8).tobytes()
            out.append((f"tail{k}@{k0}", bytes(b)))
    return out


# pmfs of pmf_to_quantized_cdf (compressai._CXX): degenerate ones
PMF_CASES = {
    "len1": [1.0],
    "len1_tiny": [1e-9],
    "len1_zero": [0.0],
    "len2": [0.3, 0.7],
    "len2_one_zero": [1.0, 0.0],
    "len2_tiny": [1e-5, 0.0],
    "all_zeros": [0.0] * 5,
    "one_entry": [0.0, 0.0, 1.0, 0.0],
    "with_nan": [0.5, float("nan"), 0.5],
    "with_inf": [0.5, float("inf")],
    "negative": [0.6, -0.1, 0.5],
    "unnormalised": [3.0, 1.0, 0.0, 7.5],
    "many_tiny": [1e-7] * 40 + [1.0],
}


# ---- the parameter head's last layer (fgmm_head.hip, fgmm_head16.hip) ----------------------------------------------------
# Every family returns (W [12 M, c_in], b [12 M], x [c_in, hw]) float32 for a given shape.  The finite families keep every partial
# sum of the fmaf chain within binary32 (no overflow in any order): sum |w x| + |b| <= 2^126.
F32_MAX = float(np.finfo(F32).max)
BF16_OVERFLOW = float.fromhex("0x1.FFp127")  # the smallest binary32 that rounds to an infinite bfloat16 (to nearest even)


def _pow2(rng, lo, hi, shape):
    """mixed signs, log-uniform magnitudes in [2^lo, 2^hi)"""
    return (np.where(rng.random(shape) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(lo, hi, shape))).astype(F32)


def _fit(W, b, x, limit):
    """x scaled by a power of two (exactly) so that sum |w x| + |b| <= limit everywhere"""
    s = (np.abs(W.astype(np.float64)) @ np.abs(x.astype(np.float64)) + np.abs(b.astype(np.float64))[:, None]).max()
    k = max(0, int(np.ceil(np.log2(s / limit)))) if s > limit else 0
    return W, b, (x * F32(2.0**-k)).astype(F32)


def _hd_ordinary(rng, M, c_in, hw):
    W = (rng.standard_normal((12 * M, c_in)) / np.sqrt(c_in)).astype(F32)
    b = rng.standard_normal(12 * M).astype(F32)
    x = rng.standard_normal((c_in, hw)).astype(F32)
    return W, b, np.where(x > 0, x, F32(0.01) * x).astype(F32)


def _hd_wide_range(rng, M, c_in, hw):
    W, b, x = _pow2(rng, -60, 60, (12 * M, c_in)), _pow2(rng, -60, 60, 12 * M), _pow2(rng, -60, 60, (c_in, hw))
    return _fit(W, b, x, 2.0**120)


def _hd_cancellation(rng, M, c_in, hw):
    """bias = -(sum w x) of position 0 rounded to binary32, and other positions near it: results far below sum |w x|"""
    W, _, x = _hd_ordinary(rng, M, c_in, hw)
    x = (x[:, :1] + F32(1e-3) * x).astype(F32)
    b = (-(W.astype(np.float64) @ x[:, 0].astype(np.float64))).astype(F32)
    return W, b, x


def _hd_huge(rng, M, c_in, hw):
    """one or two products per output near 2^125 (features of 2^61 .. 2^63 at two channels of each position), the rest ordinary"""
    W = _pow2(rng, 60, 62, (12 * M, c_in))
    x = _pow2(rng, -70, -60, (c_in, hw))
    for p in range(hw):
        x[rng.choice(c_in, min(2, c_in), replace=False), p] = _pow2(rng, 61, 63, min(2, c_in))
    return _fit(W, _pow2(rng, 100, 124, 12 * M), x, 2.0**126)


def _hd_near_bf16_overflow_features(rng, M, c_in, hw):
    """a few |x| in [0x1.FFp127, FLT_MAX] - finite, but their first bfloat16 part is infinite - at channel c_in - 1, at the last
    position, and elsewhere; weights <= 2^-4, at most one such feature per position"""
    W = (_pow2(rng, -30, -4, (12 * M, c_in))).astype(F32)
    x = _hd_ordinary(rng, M, c_in, hw)[2]
    big = np.exp2(rng.uniform(np.log2(BF16_OVERFLOW), np.log2(F32_MAX), 4)).astype(F32)
    big = np.minimum(big, F32(F32_MAX)) * np.array([1, -1, 1, -1], F32)
    big[0] = F32(BF16_OVERFLOW)
    places = [(c_in - 1, hw - 1), (0, 0), (int(rng.integers(c_in)), hw // 2), (c_in - 1, hw // 3)]
    used = set()
    for (k, p), v in zip(places, big):
        if p not in used:
            x[k, p] = v
            used.add(p)
    return W, (rng.standard_normal(12 * M) * 1e3).astype(F32), x


def _hd_subnormal(rng, M, c_in, hw):
    """subnormal features and weights beside ordinary ones: products between 2^-150 and 2^-100 among them"""
    W, b, x = _hd_ordinary(rng, M, c_in, hw)
    mx, mw = rng.random(x.shape) < 0.5, rng.random(W.shape) < 0.3
    x[mx] = _pow2(rng, -149, -126, int(mx.sum()))
    W[mw] = _pow2(rng, -149, -126, int(mw.sum()))
    return W, (b * F32(2.0**-120)).astype(F32), x


def _hd_tiny_products(rng, M, c_in, hw):
    """w x between 2^-150 and 2^-100 everywhere: the result is mostly subnormal"""
    W, x = _pow2(rng, -75, -50, (12 * M, c_in)), _pow2(rng, -75, -50, (c_in, hw))
    return W, _pow2(rng, -150, -110, 12 * M), x


def _hd_signed_zeros(rng, M, c_in, hw):
    """+-0 in the weights, the features and the bias, rows of zero weights, negative features: many chains end at -0"""
    W, b, x = _hd_ordinary(rng, M, c_in, hw)
    W[rng.random(W.shape) < 0.5] = 0.0
    W[rng.random(W.shape) < 0.3] = -0.0
    W[rng.random(12 * M) < 0.6] = np.where(rng.random(c_in) < 0.5, F32(0.0), F32(-0.0))  # zero rows, both signs
    b = np.where(rng.random(12 * M) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
    x = -np.abs(x)
    x[rng.random(x.shape) < 0.2] = -0.0
    x[rng.random(x.shape) < 0.1] = 0.0
    return W, b, x


def _hd_dead_rows(rng, M, c_in, hw):
    W, b, x = _hd_ordinary(rng, M, c_in, hw)
    dead = rng.random(12 * M) < 0.4
    W[dead] = 0.0
    b[dead[: 12 * M] & (rng.random(12 * M) < 0.5)] = 0.0
    return W, b, x


def _hd_nonfinite_features(rng, M, c_in, hw):
    """NaN and +-inf features, at input channel c_in - 1, at the last position (a last, partial position tile) and elsewhere"""
    W, b, x = _hd_ordinary(rng, M, c_in, hw)
    vals = [np.nan, np.inf, -np.inf]
    x[c_in - 1, hw - 1] = np.inf
    x[0, 0] = np.nan
    if hw > 2:
        x[c_in - 1, 1] = -np.inf
        x[int(rng.integers(c_in)), hw // 2] = vals[int(rng.integers(3))]
    return W, b, x


def _hd_nonfinite_weights(rng, M, c_in, hw):
    """NaN and +-inf weights (column c_in - 1 included) and one infinite bias"""
    W, b, x = _hd_ordinary(rng, M, c_in, hw)
    W[0, c_in - 1] = np.inf
    W[12 * M - 1, 0] = np.nan
    W[int(rng.integers(12 * M)), int(rng.integers(c_in))] = -np.inf
    b[6 * M] = -np.inf
    return W, b, x


HEAD_FAMILIES = {
    "ordinary": _hd_ordinary,
    "wide_range": _hd_wide_range,
    "cancellation": _hd_cancellation,
    "huge": _hd_huge,
    "near_bf16_overflow_features": _hd_near_bf16_overflow_features,
    "subnormal": _hd_subnormal,
    "tiny_products": _hd_tiny_products,
    "signed_zeros": _hd_signed_zeros,
    "dead_rows": _hd_dead_rows,
    "nonfinite_features": _hd_nonfinite_features,
    "nonfinite_weights": _hd_nonfinite_weights,
}
HEAD_NONFINITE = ("nonfinite_features", "nonfinite_weights")  # the exact result is NaN or +-inf somewhere
# outside the bf16x6 form's domain (include/flashgmm_amd.h FGMM_HEAD_BF16X6): features it hands to the exact form, weights it refuses
HEAD_BF16_FEATURES_OUT = ("near_bf16_overflow_features", "nonfinite_features")
HEAD_BF16_WEIGHTS_OUT = ("nonfinite_weights",)


def head_case(family: str, M: int, c_in: int, hw: int, seed: int = 0):
    """-> (W [12 M, c_in], b [12 M], x [c_in, hw]) float32, contiguous"""
    W, b, x = HEAD_FAMILIES[family](_rng(f"head/{family}/{M}/{c_in}/{hw}", seed), M, c_in, hw)
    return tuple(np.ascontiguousarray(a, F32) for a in (W, b, x))
