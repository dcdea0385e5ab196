"""The arithmetic of include/flashgmm_amd.h section 3g - the entropy model's forward(): likelihood, pass-through rules, gradients - in
a few lines of torch, in binary32 or binary64, and the seeded corpus the likelihood tests share.

``forward`` / ``backward`` follow the header's formulas operation by operation (k ascending, separate multiply and add), so the
float32 evaluation is the kernel's arithmetic in torch operations.  The float64 yardstick the GPU tests measure both against is
``forward`` for likelihoods and ``reference_gradients`` for gradients (autograd through the same forward in the reference's sequence of
operations); tests/test_likelihood_cpu.py ties both to the reference's own class through tests/golden/g10_likelihood.npz (written by
tests/golden/make_golden_likelihood.py), and holds ``backward`` in float64 to them up to the rounding of the terms it cancels.

The corpus is 2048 latents laid out as y [1, 8, 16, 16] and planes [1, 32, 16, 16] (plane k of channel c is channel k * 8 + c), so
the same arrays go through the public interface.  Channel by channel:

    0-1 (a) typical         sigma = exp(U(-3, 2.5)) times a per-component factor, mu within a few sigma of y, pi a softmax
    2   (b) scale bound     sigma in {0.02, the binary32 below sb, sb, the binary32 above sb}
    3   (c) deep tail       |y - mu_k| >= 45 sigma_k + 1 for every k: L underflows far below 1e-9
    4   (d) exact hits      y an integer and mu_k == y exactly for one k: the sign-0 case (with and without rounding)
    5   (e) wide            sigma in [64, 3000]
    6   (f) cancellation    sigma ~ 256 with |y - mu| < 1
    7   (g) unconstrained   weights with a negative component, or summing to 1.7
"""
import math

import numpy as np
import torch

SB, LB = 0.11, 1e-9  # the reference's defaults (entropy_models.py:113, 636); the kernel and the reference hold them as binary32
LN2F = float.fromhex("0x1.62e430p-1")
SEED = 20261019
SHAPE = (1, 8, 16, 16)
REGIONS = {"a": (0, 512), "b": (512, 768), "c": (768, 1024), "d": (1024, 1280), "e": (1280, 1536), "f": (1536, 1792), "g": (1792, 2048)}
GRADS = ("dy", "dscales", "dmeans", "dweights")


def f32(x):
    """a Python float -> the binary32 nearest to it, as a Python float"""
    return float(np.float32(x))


def _k(t, K=4):
    """planes [B, K*M, h, w] -> [B, K, M, h, w]"""
    return t.reshape(t.shape[0], K, t.shape[1] // K, *t.shape[2:])


def forward(y, scales, means, weights, rnd, sb=SB, lb=LB, dtype=torch.float32):
    """-> dict of v, the likelihood ``out`` and what ``backward`` needs.  Inputs are converted to ``dtype`` exactly (they hold binary32
    or narrower values); the bounds are the binary32 values of ``sb`` / ``lb`` widened; the constants are ``dtype``'s own."""
    y, sg, mu, pi = y.to(dtype), _k(scales.to(dtype)), _k(means.to(dtype)), _k(weights.to(dtype))
    sbt, lbt = torch.tensor(f32(sb), dtype=dtype, device=y.device), torch.tensor(f32(lb), dtype=dtype, device=y.device)
    c = float(-(2 ** -0.5))  # torch rounds a Python scalar to the tensor's dtype: (float)(-(2^-0.5)) in binary32
    v = torch.round(y) if rnd else y
    s = torch.max(sg, sbt)  # keeps a NaN sigma
    a = torch.abs(v.unsqueeze(1) - mu)
    xu, xl = (0.5 - a) / s, (-0.5 - a) / s
    p = 0.5 * torch.erfc(c * xu) - 0.5 * torch.erfc(c * xl)
    L = torch.zeros_like(y)
    for k in range(4):
        L = L + p[:, k] * pi[:, k]
    out = torch.max(L, lbt) if lb > 0 else L
    return dict(v=v, out=out, L=L, p=p, s=s, xu=xu, xl=xl, sg=sg, mu=mu, pi=pi, sbt=sbt, lbt=lbt, lb=lb, rnd=rnd, dtype=dtype)


def g_from_bits(out, g_bits):
    """the upstream gradient the kernel forms from a scalar on the item's bit count: -gb / (out * ln2f), binary32"""
    gb = torch.tensor(f32(g_bits), dtype=torch.float32, device=out.device)
    return -gb / (out * torch.tensor(LN2F, dtype=torch.float32, device=out.device))


def backward(f, g):
    """the explicit gradients of section 3g at the upstream gradient ``g`` (w.r.t. ``out``) -> dict dy [B, M, h, w] and dscales / dmeans /
    dweights [B, K*M, h, w], plus ``pass_like`` [B, M, h, w] and ``pass_scale`` [B, K*M, h, w], the pass-through decisions"""
    dt = f["dtype"]
    g = g.to(dt)
    inv = 1.0 / math.sqrt(2.0 * math.pi)
    phi = lambda x: torch.exp(-0.5 * x * x) * inv  # noqa: E731
    v, p, s, xu, xl, sg, mu, pi = (f[n] for n in ("v", "p", "s", "xu", "xl", "sg", "mu", "pi"))
    zero = torch.zeros((), dtype=dt, device=g.device)
    pass_like = (f["L"] >= f["lbt"]) | (g < 0) | (f["lb"] <= 0)
    gL = torch.where(pass_like, g, zero).unsqueeze(1)
    fu, fl = phi(xu), phi(xl)
    dpi = gL * p
    da = -pi * (fu - fl) / s
    sgn = (v.unsqueeze(1) > mu).to(dt) - (v.unsqueeze(1) < mu).to(dt)
    dmu = -gL * da * sgn
    t = gL * da * sgn
    dv = torch.zeros_like(v)
    for k in range(4):
        dv = dv + t[:, k]
    G = gL * (-pi * (fu * xu - fl * xl) / s)
    pass_scale = (sg >= f["sbt"]) | (G < 0)
    dsg = torch.where(pass_scale, G, zero)
    flat = lambda x: x.reshape(x.shape[0], -1, *x.shape[3:])  # noqa: E731
    return dict(dy=torch.zeros_like(dv) if f["rnd"] else dv, dscales=flat(dsg), dmeans=flat(dmu), dweights=flat(dpi), pass_like=pass_like,
                pass_scale=flat(pass_scale))


class _LowerBound(torch.autograd.Function):
    """torch.max(x, bound) with the reference's gradient (bound_ops.py:36-42), for `autograd_forward` below"""

    @staticmethod
    def forward(ctx, x, bound):
        ctx.save_for_backward(x, bound)
        return torch.max(x, bound)

    @staticmethod
    def backward(ctx, g):
        x, bound = ctx.saved_tensors
        return ((x >= bound) | (g < 0)) * g, None


def autograd_forward(v, scales, means, weights, sb=SB, lb=LB):
    """the float32 formula as torch eager evaluates it WITH autograd (what scripts/likelihood_time.py times): the reference's own
    sequence of operations, entropy_models.py:720-737, 774-808, on the tensors as they are"""
    sbt, lbt = (torch.tensor(f32(b), dtype=v.dtype, device=v.device) for b in (sb, lb))
    M = v.size(1)
    like = torch.zeros_like(v)
    for k in range(4):
        s = _LowerBound.apply(scales[:, M * k:M * (k + 1)], sbt)
        a = torch.abs(v - means[:, M * k:M * (k + 1)])
        c = float(-(2 ** -0.5))
        p = 0.5 * torch.erfc(c * ((0.5 - a) / s)) - 0.5 * torch.erfc(c * ((-0.5 - a) / s))
        like = like + p * weights[:, M * k:M * (k + 1)]
    return _LowerBound.apply(like, lbt)


def reference_gradients(y, scales, means, weights, g, rnd=False, sb=SB, lb=LB, dtype=torch.float64):
    """The float64 yardstick for GRADIENTS: torch's autograd through ``autograd_forward`` - section 3g's forward in the reference's own
    sequence of operations, with the reference's two pass-through rules - at the upstream gradient g.  -> (likelihood, dict of dy,
    dscales, dmeans, dweights; dy zero with rounding).  On the fixture's inputs it gives the reference's own class's gradients bit for
    bit (tests/test_likelihood_cpu.py).  ``backward`` above, the explicit formulas the kernel runs, is the same derivative grouped
    differently: (phi(xu) - phi(xl)) / s where autograd forms phi(xu) / s and phi(xl) / s apart, so in float64 the two differ by
    rounding errors of the terms that cancel - up to 2.4e-7 of the result on the corpus, 1e-16 of the terms."""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (y, scales, means, weights)]
    like = autograd_forward(torch.round(leaves[0]) if rnd else leaves[0], *leaves[1:], sb, lb)
    like.backward(g.to(dtype))
    return like.detach(), dict(zip(GRADS, (t.grad for t in leaves)))


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------
def _softmax(rng, n):
    lg = rng.standard_normal((n, 4))
    e = np.exp(lg - lg.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def corpus(seed=SEED):
    """-> y, scales, means, weights, g as float32 arrays in the public layout ([1, 8, 16, 16] / [1, 32, 16, 16]); rows REGIONS[r] of the
    flat latent (channel-major) belong to region r"""
    rng = np.random.default_rng(seed)
    n = 2048
    y = np.zeros(n, np.float32)
    sg, mu, pi = (np.zeros((n, 4), np.float32) for _ in range(3))

    def typical(lo, hi, sigma):
        m = hi - lo
        base = rng.standard_normal(m) * 4
        mu[lo:hi] = (base[:, None] + rng.standard_normal((m, 4)) * sigma * 1.5).astype(np.float32)
        y[lo:hi] = (base + rng.standard_normal(m) * sigma.mean(1) * 1.5).astype(np.float32)
        sg[lo:hi] = sigma.astype(np.float32)
        pi[lo:hi] = _softmax(rng, m).astype(np.float32)

    lo, hi = REGIONS["a"]
    typical(lo, hi, np.exp(rng.uniform(-3, 2.5, hi - lo))[:, None] * rng.uniform(0.5, 2.0, (hi - lo, 4)))
    lo, hi = REGIONS["b"]
    sb32 = np.float32(SB)
    edge = np.array([0.02, np.nextafter(sb32, np.float32(0)), sb32, np.nextafter(sb32, np.float32(1))], np.float32)
    typical(lo, hi, edge[rng.integers(0, 4, (hi - lo, 4))].astype(np.float64))
    mu[lo:hi] = (y[lo:hi, None] + rng.uniform(-0.9, 0.9, (hi - lo, 4))).astype(np.float32)  # within reach of sigma ~ 0.11: G_k of either sign
    lo, hi = REGIONS["c"]
    typical(lo, hi, np.exp(rng.uniform(-3, 1.0, (hi - lo, 4))))
    far = (45.0 * sg[lo:hi] + 1.0) * rng.uniform(1.05, 2.0, (hi - lo, 4)) * rng.choice([-1.0, 1.0], (hi - lo, 4))
    mu[lo:hi] = (np.round(y[lo:hi, None]) + np.sign(far) * 0.5 + far).astype(np.float32)
    lo, hi = REGIONS["d"]
    typical(lo, hi, np.exp(rng.uniform(-2, 1.5, (hi - lo, 4))))
    y[lo:hi] = np.round(y[lo:hi])
    hit = rng.integers(0, 4, hi - lo)
    mu[np.arange(lo, hi), hit] = y[lo:hi]
    lo, hi = REGIONS["e"]
    typical(lo, hi, np.exp(rng.uniform(np.log(64.0), np.log(3000.0), (hi - lo, 4))))
    lo, hi = REGIONS["f"]
    typical(lo, hi, 256.0 * (1.0 + rng.uniform(-0.01, 0.01, (hi - lo, 4))))
    mu[lo:hi] = (y[lo:hi, None] + rng.uniform(-0.99, 0.99, (hi - lo, 4))).astype(np.float32)
    lo, hi = REGIONS["g"]
    typical(lo, hi, np.exp(rng.uniform(-1.5, 2.0, (hi - lo, 4))))
    half = (lo + hi) // 2
    pi[lo:half] = (pi[lo:half].astype(np.float64) * 1.7).astype(np.float32)
    neg = rng.integers(0, 4, hi - half)
    pi[np.arange(half, hi), neg] = (-0.25 * pi[np.arange(half, hi), neg]).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp(rng.uniform(-2, 2, n))).astype(np.float32)
    g[g == 0] = 1.0
    planes = lambda r: np.ascontiguousarray(r.reshape(8, 256, 4).transpose(2, 0, 1)).reshape(1, 32, 16, 16)  # noqa: E731
    return y.reshape(SHAPE), planes(sg), planes(mu), planes(pi), g.reshape(SHAPE)


def region_mask(name):
    m = np.zeros(2048, bool)
    m[REGIONS[name][0]:REGIONS[name][1]] = True
    return m.reshape(SHAPE)


def plane_mask(name):
    """the region's rows in the [1, 32, 16, 16] layout of the parameter planes and their gradients"""
    return np.tile(region_mask(name), (1, 4, 1, 1))


def near_bound(like64, lb=LB, rel=1e-3):
    """rows whose float64 L lies within `rel` relative of lb: a float32 and a float64 evaluation may fall on different sides of the bound"""
    return np.abs(like64 - f32(lb)) <= rel * f32(lb)
