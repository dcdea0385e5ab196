"""The arithmetic of include/flashgmm_amd.h section 3i - centroid reconstruction of a decoded latent - in a few lines of torch, over
tests/like_ref.py (section 3g's terms and its corpus, imported, not edited).

``centroid(..., dtype=torch.float64, form="closed")`` is the YARDSTICK: the closed form of the bin's conditional mean under the mixture,
no series, in binary64.  ``centroid(..., dtype=torch.float32)`` restates the header's binary32 sequence operation by operation (k
ascending, separate multiply and add, the narrow / wide select), so on the GPU it is the kernel's arithmetic in torch operations - the
allowance the GPU tests grant the kernel.  ``form="series"`` evaluates the wide form on every component (the CPU test holds it to the
closed form).  ``near`` names the rows on which two precisions may legitimately decide ``keep`` differently, ``sample`` draws latents
from their own mixtures.

Per component, with t = v - mu, a = |t|, s = max(sigma, sb), xu = (0.5 - a)/s, xl = (-0.5 - a)/s, p = Phi(xu) - Phi(xl): the bin's first
moment about v is -sign(t) * m with m = a*p - s*(phi(xu) - phi(xl)); expanded in h = 1/(2s) at xb = a/s,
m = a*phi(xb)*h^3*(2/3 + h^2 (xb^2 - 3)/15 + h^4 ((xb^2 - 10) xb^2 + 15)/420 + h^6 He7(xb)/(xb 22680) + ...)."""
import math

import numpy as np
import torch

from tests import like_ref as R

P_MIN = 2.0 ** -16  # the Python default: the coder's resolution
WIDE = 2.0          # a component with s >= WIDE takes the series


def _phi(x):
    return torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def centroid(y, scales, means, weights, sb=R.SB, p_min=P_MIN, dtype=torch.float32, form="header"):
    """-> dict of v, L, off, keep, rec ``[B, M, h, w]`` and, per component ``[B, K, M, h, w]``, m and what the tests bound errors with.
    Inputs are converted to ``dtype`` exactly; sb and p_min are their binary32 values widened; the constants are ``dtype``'s own.
    ``form``: "header" (the select of section 3i), "closed" (the literal form everywhere) or "series" (the wide form everywhere)"""
    f = R.forward(y, scales, means, weights, rnd=True, sb=sb, lb=0.0, dtype=dtype)
    v, p, s, xu, xl, mu, pi, L = (f[n] for n in ("v", "p", "s", "xu", "xl", "mu", "pi", "L"))
    t = v.unsqueeze(1) - mu
    a = torch.abs(t)
    sgn = (t > 0).to(dtype) - (t < 0).to(dtype)
    fu, fl = _phi(xu), _phi(xl)
    narrow = a * p - s * (fu - fl)
    h = 0.5 / s
    xb = a * (h + h)
    h2, x2 = h * h, xb * xb
    q = ((2.0 / 3.0) + (h2 * (x2 - 3.0)) * (1.0 / 15.0)) + ((h2 * h2) * ((x2 - 10.0) * x2 + 15.0)) * (1.0 / 420.0)
    wide = ((a * _phi(xb)) * (h * h2)) * q
    is_wide = s >= WIDE
    m = {"header": torch.where(is_wide, wide, narrow), "closed": narrow, "series": wide}[form]
    N = torch.zeros_like(v)
    for k in range(4):
        N = N + (pi[:, k] * sgn[:, k]) * m[:, k]
    off = (-N) / L
    keep = (L >= torch.tensor(R.f32(p_min), dtype=dtype, device=v.device)) & (torch.abs(off) <= 0.5) & torch.all(s < float("inf"), dim=1)
    rec = torch.where(keep, v + off, v)
    u = 0.5 * torch.erfc(float(-(2 ** -0.5)) * xu)  # (p = u - l: u + l is 2 u - p)
    return dict(v=v, L=L, off=off, keep=keep, rec=rec, m=m, a=a, s=s, p=p, pi=pi, xb=xb, h=h, is_wide=is_wide, u_plus_l=2.0 * u - p, f_plus=fu + fl)


def near(L64, off64, p_min=P_MIN, rel=1e-3):
    """rows whose float64 L lies within ``rel`` relative of p_min, or whose float64 |off| within ``rel`` of 0.5: a binary32 and a binary64
    evaluation may decide ``keep`` differently there"""
    L64, off64 = np.asarray(L64, np.float64), np.asarray(off64, np.float64)
    with np.errstate(invalid="ignore"):
        return (np.abs(L64 / R.f32(p_min) - 1.0) < rel) | (np.abs(np.abs(off64) - 0.5) < rel)


def allowance(c64, ulps=8.0, eps=2.0 ** -24):
    """Per row, what a correct binary32 evaluation of section 3i may be off by in ``off`` - from the condition of the sum, not from any
    code's result.  Each of u, l, phi(xu), phi(xl) carries a relative error of a few ulps (the library's erfc and exp, the rounding of
    their arguments), so a narrow component's m_k = a p - s (phi(xu) - phi(xl)) is off by up to ulps*eps*(a (u + l) + s (phi(xu) +
    phi(xl))) however much of it cancels; a wide component's series has no cancellation and is off by ulps*eps*(1 + xb^2 / 2)*|m_k|
    (the exponent's rounding is amplified by xb^2 / 2); L is off by ulps*eps*sum |pi_k| (u + l).  With off = -N / L:
    |d off| <= ulps*eps * (sum_k |pi_k| cond_k + |off| sum_k |pi_k| (u_k + l_k)) / |L|, plus one ulp of 0.5 for the final operations."""
    pi, ul = torch.abs(c64["pi"]), c64["u_plus_l"]
    cond = torch.where(c64["is_wide"], (1.0 + 0.5 * c64["xb"] ** 2) * torch.abs(c64["m"]), c64["a"] * ul + c64["s"] * c64["f_plus"])
    return (ulps * eps) * ((pi * cond).sum(1) + torch.abs(c64["off"]) * (pi * ul).sum(1)) / torch.abs(c64["L"]) + 2.0 ** -24


def series_remainder(c64):
    """A bound of what the three-term series leaves out, per component, in m's units.  The moment is a phi(xb) sum_n h^(n+2) He_n(xb) /
    (xb (n+2) n!/2) over odd n; the series stops after n = 5.  The bound is the n = 7 term itself, a phi(xb) h^9 |xb^6 - 21 xb^4 +
    105 xb^2 - 105| / 22680, plus twice the n = 9 term with its monomials taken in absolute value, a phi(xb) h^11 (xb^8 + 36 xb^6 +
    378 xb^4 + 1260 xb^2 + 945) / 1995840 (where He_7 has a root the n = 9 term leads; each further term is below a fifth of the one
    before at h <= 1/4, xb <= 4.5, so twice the n = 9 bound covers the rest)"""
    x2, front = c64["xb"] ** 2, c64["a"] * _phi(c64["xb"])
    t7 = front * c64["h"] ** 9 * torch.abs(((x2 - 21.0) * x2 + 105.0) * x2 - 105.0) / 22680.0
    t9 = front * c64["h"] ** 11 * ((((x2 + 36.0) * x2 + 378.0) * x2 + 1260.0) * x2 + 945.0) / 1995840.0
    return t7 + 2.0 * t9


def quadrature(y, scales, means, weights, rows, sb=R.SB, points=20001):
    """the conditional mean offset of the bin of round(y) by composite Simpson on ``points`` nodes of the mixture DENSITY, binary64, for
    the flat latent indices ``rows`` of arrays in the public layout -> (off, L)"""
    yf = np.asarray(y, np.float64).reshape(-1)
    K = [np.asarray(a, np.float64).reshape(4, -1) for a in (scales, means, weights)]
    x = np.linspace(-0.5, 0.5, points)
    wts = np.ones(points)
    wts[1:-1:2], wts[2:-1:2] = 4.0, 2.0
    wts *= (x[1] - x[0]) / 3.0
    off, like = [], []
    for i in rows:
        v = np.round(yf[i])
        s = np.maximum(K[0][:, i], R.f32(sb))[:, None]
        z = (v + x[None, :] - K[1][:, i][:, None]) / s
        dens = (K[2][:, i][:, None] * np.exp(-0.5 * z * z) / (s * math.sqrt(2.0 * math.pi))).sum(0)
        like.append(float((wts * dens).sum()))
        off.append(float((wts * dens * x).sum()) / like[-1])
    return np.array(off), np.array(like)


def sample(seed=R.SEED + 7, M=4, h=32, w=32, sb=R.SB):
    """latents drawn from their own mixtures, region (a)'s recipe for the parameters (tests/like_ref.py): -> y [1, M, h, w] (NOT rounded),
    scales, means, weights [1, 4M, h, w], float32 arrays in the public layout.  Component k of a latent is drawn with probability pi_k,
    then y = mu_k + max(sigma_k, sb) * N(0, 1): the density section 3i takes the centroid under"""
    rng = np.random.default_rng(seed)
    n = M * h * w
    sigma = (np.exp(rng.uniform(-3, 2.5, n))[:, None] * rng.uniform(0.5, 2.0, (n, 4))).astype(np.float32)
    base = rng.standard_normal(n) * 4
    mu = (base[:, None] + rng.standard_normal((n, 4)) * sigma * 1.5).astype(np.float32)
    lg = rng.standard_normal((n, 4))
    pi = (np.exp(lg) / np.exp(lg).sum(1, keepdims=True)).astype(np.float32)
    cdf = np.cumsum(pi.astype(np.float64), 1)
    k = np.minimum((rng.uniform(0, 1, n)[:, None] * cdf[:, -1:] > cdf).sum(1), 3)
    at = np.arange(n)
    y = (mu[at, k].astype(np.float64) + np.maximum(sigma[at, k], np.float32(sb)).astype(np.float64) * rng.standard_normal(n)).astype(np.float32)
    planes = lambda r: np.ascontiguousarray(r.reshape(M, h * w, 4).transpose(2, 0, 1)).reshape(1, 4 * M, h, w)  # noqa: E731
    return y.reshape(1, M, h, w), planes(sigma), planes(mu), planes(pi)
