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

``corpus(sb=...)`` rebuilds region (b) around another scale bound, ``edge_inputs`` plants non-finite and degenerate values in regions
(a) and (e).  ``launch_form`` restates the launcher's choice of positions per lane and grid (fgmm_like.cpp, LikeShape), and ``CASES``
lists the form every GPU case of the two likelihood modules is there for.
"""
import math

import numpy as np
import torch

SB, LB = 0.11, 1e-9  # the reference's defaults (entropy_models.py:113, 636); the kernel and the reference hold them as binary32
LN2F = float.fromhex("0x1.62e430p-1")
SEED = 20261019
BOUNDS = [(0.11, 0.0), (0.5, 1e-9), (2.0 ** -10, 1e-4), (0.11, 0.5)]  # the (scale_bound, likelihood_bound) settings run beside the defaults
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
    """the upstream gradient the kernel forms from a scalar on the item's bit count: -gb / (out * ln2f), binary32; 0 for a latent that
    is left out of the sum (out NaN, infinite or <= 0)"""
    gb = torch.tensor(f32(g_bits), dtype=torch.float32, device=out.device)
    g = -gb / (out * torch.tensor(LN2F, dtype=torch.float32, device=out.device))
    return torch.where(counts(out), g, torch.zeros((), dtype=torch.float32, device=out.device))


def counts(out):
    """the latents that take part in bits_q: a finite out > 0 (false for NaN)"""
    return (out > 0) & (out < float("inf"))


def backward(f, g):
    """the explicit gradients of section 3g at the upstream gradient ``g`` (w.r.t. ``out``) -> dict dy [B, M, h, w] and dscales / dmeans /
    dweights [B, K*M, h, w], plus ``pass_like`` [B, M, h, w] and ``pass_scale`` [B, K*M, h, w], the pass-through decisions, and ``G``
    [B, K*M, h, w], the gradient arriving at s_k before its rule"""
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
                pass_scale=flat(pass_scale), G=flat(G))


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
    return _LowerBound.apply(like, lbt) if lb > 0 else like  # (lb = 0: no bound, as `forward` and the header have it)


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


def corpus(seed=SEED, sb=SB):
    """-> y, scales, means, weights, g as float32 arrays in the public layout ([1, 8, 16, 16] / [1, 32, 16, 16]); rows REGIONS[r] of the
    flat latent (channel-major) belong to region r.  ``sb``: the scale bound region (b) is built around (the draws do not depend on it)"""
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
    sb32 = np.float32(sb)
    edge = np.array([0.02 * (sb / SB), np.nextafter(sb32, np.float32(0)), sb32, np.nextafter(sb32, np.float32(1))], np.float32)
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
    """rows whose float64 L lies within `rel` relative of lb: a float32 and a float64 evaluation may fall on different sides of the bound
    (lb = 0: there is no bound to fall either side of, no row is near it)"""
    if lb <= 0:
        return np.zeros(np.shape(like64), bool)
    return np.abs(like64 - f32(lb)) <= rel * f32(lb)


# ---- the launcher's decisions ---------------------------------------------------------------------------------------------------------
def form_item(hw, stride_c, stride_k, planes, rest):
    """one item as ``launch_form`` reads it: ``planes`` the byte addresses of scales, means and weights, ``rest`` those of y and of every
    output (and g_like) of the call, 0 for NULL"""
    return dict(hw=int(hw), stride_c=int(stride_c), stride_k=int(stride_k), planes=tuple(int(p) for p in planes), rest=tuple(int(p) for p in rest))


def launch_form(items, two_byte, backward):
    """``LikeShape`` (fgmm_like.cpp) restated: -> (vec, linear), the positions per lane and the grid of the ONE launch that serves every
    item.  4 per lane needs hw, stride_c and stride_k multiples of 4, planes aligned to 4 elements, y and every other pointer to 16
    bytes; 8 per lane (two-byte planes, forward only) the same with 8 and planes at 16 bytes.  Both are ANDed over the items.  The
    linear grid needs every hw a multiple of 64 * vec; 8 falls back to 4 where that, and only that, keeps the linear grid."""
    vec4 = vec8 = True
    for it in items:
        strides = (it["hw"], it["stride_c"], it["stride_k"])
        ok4 = all(x % 4 == 0 for x in strides) and all(p % (8 if two_byte else 16) == 0 for p in it["planes"]) and all(p % 16 == 0 for p in it["rest"])
        vec4 = vec4 and ok4
        vec8 = vec8 and ok4 and two_byte and all(x % 8 == 0 for x in strides) and all(p % 16 == 0 for p in it["planes"])
    vec = (8 if vec8 and not backward else 4) if vec4 else 1
    fills = lambda v: all(it["hw"] % (64 * v) == 0 for it in items)  # noqa: E731
    if vec == 8 and not fills(8) and fills(4):
        vec = 4
    return vec, fills(vec)


# ---- non-finite inputs ------------------------------------------------------------------------------------------------------------------
KINDS = ("nan_sigma", "nan_weight", "y_pinf", "y_ninf", "mu_pinf", "y_mu_pinf", "sigma_pinf", "sigma_zero", "weight_pinf")


def edge_inputs(seed=SEED):
    """-> (y, scales, means, weights, g, planted): ``corpus(seed)`` with non-finite or degenerate values planted at distinct latents of
    regions (a) and (e), four of every kind in each; ``planted`` lists (kind, flat latent index, component).  Everything planted is
    representable in bfloat16."""
    y, sg, mu, pi, g = (a.copy() for a in corpus(seed))
    rng = np.random.default_rng(seed + 1)
    rows = np.concatenate([lo + rng.choice(hi - lo, 4 * len(KINDS), replace=False) for lo, hi in (REGIONS["a"], REGIONS["e"])])
    yf, plane = y.reshape(-1), lambda a, k: a.reshape(4, -1)[k]  # noqa: E731
    planted = []
    for j, i in enumerate(rows.tolist()):
        kind, k = KINDS[j % len(KINDS)], int(rng.integers(0, 4))
        planted.append((kind, i, k))
        if kind == "nan_sigma":
            plane(sg, k)[i] = np.nan
        elif kind == "nan_weight":
            plane(pi, k)[i] = np.nan
        elif kind in ("y_pinf", "y_ninf"):
            yf[i] = np.inf if kind == "y_pinf" else -np.inf
        elif kind == "mu_pinf":
            plane(mu, k)[i] = np.inf
        elif kind == "y_mu_pinf":
            yf[i] = plane(mu, k)[i] = np.inf
        elif kind == "sigma_pinf":
            plane(sg, k)[i] = np.inf
        elif kind == "sigma_zero":
            plane(sg, k)[i] = 0.0
        else:  # the one way to out = +inf (p_k > 0) - or to NaN, where p_k is 0
            plane(pi, k)[i] = np.inf
    return y, sg, mu, pi, g, planted


def planted_mask(planted):
    m = np.zeros(2048, bool)
    m[[i for _, i, _ in planted]] = True
    return m.reshape(SHAPE)


def classes(x):
    """per element: 0 NaN, 1 +inf, 2 -inf, 3 zero of either sign, 4 any other finite value"""
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    c = np.full(x.shape, 4, np.int8)
    c[x == 0] = 3
    c[np.isneginf(x)] = 2
    c[np.isposinf(x)] = 1
    c[np.isnan(x)] = 0
    return c


# ---- the forms the GPU cases are there for ------------------------------------------------------------------------------------------------
def dense_item(M, hw, planes_off=0, y_off=0, rest_off=(0,), stride_c=None, stride_k=None):
    """a ``form_item`` of dense planes (or of the given strides); the offsets are bytes past a 16-byte boundary"""
    stride_c = hw if stride_c is None else stride_c
    return form_item(hw, stride_c, M * stride_c if stride_k is None else stride_k, (planes_off,) * 3, (y_off,) + tuple(rest_off))


LIN, TILED = True, False
ALL, TWO, F32_BF16 = ("f32", "f16", "bf16"), ("f16", "bf16"), ("f32", "bf16")
# (case, plane types, items, the forward launch's (vec, linear), the backward launch's).  "old_": the cases of tests/test_gpu_likelihood.py;
# the others are tests/test_gpu_likelihood_edges.py's, which asserts the same forms on the addresses it really passes.
CASES = [
    ("old_corpus", ("f32",), [dense_item(8, 256)], (4, LIN), (4, LIN)),
    ("old_hw255", ("f32",), [dense_item(4, 255)], (1, TILED), (1, TILED)),
    ("old_M3_hw768", ("f32",), [dense_item(3, 768)], (4, LIN), (4, LIN)),
    ("old_B3_hw64", ("f32",), [dense_item(2, 64)] * 3, (4, TILED), (4, TILED)),
    ("old_offset_hw256", ("f32",), [dense_item(8, 256, 4, 4, (4,))], (1, LIN), (1, LIN)),
    ("old_hw256", TWO, [dense_item(4, 256)], (4, LIN), (4, LIN)),
    ("old_hw264", TWO, [dense_item(4, 264)], (8, TILED), (4, TILED)),
    ("old_hw252", TWO, [dense_item(4, 252)], (4, TILED), (4, TILED)),
    ("old_hw512", TWO, [dense_item(2, 512)] * 2, (8, LIN), (4, LIN)),
    # a. two-byte planes, one position per lane
    ("a_hw35", TWO, [dense_item(3, 35)], (1, TILED), (1, TILED)),
    ("a_planes_off", TWO, [dense_item(3, 64, planes_off=2)] * 2, (1, LIN), (1, LIN)),
    ("a_y_off", TWO, [dense_item(4, 256, y_off=4)], (1, LIN), (1, LIN)),
    # b. batches whose items differ
    ("b_unequal", ("f32",), [dense_item(2, 256), dense_item(5, 256), dense_item(1, 512)], (4, LIN), (4, LIN)),
    ("b_unequal", ("bf16",), [dense_item(2, 256), dense_item(5, 256), dense_item(1, 512)], (4, LIN), (4, LIN)),  # 8 -> 4: hw 256 does not fill 8
    ("b_vec8", ("f32",), [dense_item(2, 512), dense_item(3, 1024)], (4, LIN), (4, LIN)),
    ("b_vec8", ("bf16",), [dense_item(2, 512), dense_item(3, 1024)], (8, LIN), (4, LIN)),
    ("b_y_off", F32_BF16, [dense_item(2, 256), dense_item(2, 256, y_off=4)], (1, LIN), (1, LIN)),
    ("b_out_off", F32_BF16, [dense_item(2, 256, rest_off=(0, 4))], (1, LIN), (1, LIN)),
    ("b_M0", F32_BF16, [dense_item(0, 256), dense_item(2, 256)], (4, LIN), (4, LIN)),
    ("b_hw0", F32_BF16, [dense_item(2, 0), dense_item(2, 256)], (4, LIN), (4, LIN)),
    ("b_rate_only", F32_BF16, [dense_item(2, 256)], (4, LIN), (4, LIN)),
    # c. strided planes: M 3, hw 64 and 35; chunks of [2, 12M, h, w], every second channel of [2, 8M, h, w], every second item of [4, 4M, h, w]
    ("c_chunk_hw64", ("f32",), [dense_item(3, 64)] * 2, (4, TILED), (4, TILED)),
    ("c_chunk_hw64", ("bf16",), [dense_item(3, 64)] * 2, (8, TILED), (4, TILED)),
    ("c_every2_hw64", ("f32",), [dense_item(3, 64, stride_c=128)] * 2, (4, TILED), (4, TILED)),
    ("c_every2_hw64", ("bf16",), [dense_item(3, 64, stride_c=128)] * 2, (8, TILED), (4, TILED)),
    ("c_batch2_hw64", ("f32",), [dense_item(3, 64)] * 2, (4, TILED), (4, TILED)),
    ("c_batch2_hw64", ("bf16",), [dense_item(3, 64)] * 2, (8, TILED), (4, TILED)),
    ("c_chunk_hw35", F32_BF16, [dense_item(3, 35)] * 2, (1, TILED), (1, TILED)),
    ("c_every2_hw35", F32_BF16, [dense_item(3, 35, stride_c=70)] * 2, (1, TILED), (1, TILED)),
    ("c_batch2_hw35", F32_BF16, [dense_item(3, 35)] * 2, (1, TILED), (1, TILED)),
    ("c_ctypes_hw64", ("f32",), [dense_item(3, 64, stride_c=128)], (4, TILED), (4, TILED)),
    ("c_ctypes_hw64", ("bf16",), [dense_item(3, 64, stride_c=128)], (8, TILED), (4, TILED)),
    ("c_ctypes_hw35", F32_BF16, [dense_item(3, 35, stride_c=70)], (1, TILED), (1, TILED)),
    # d. partial outputs
    ("d_hw256", ("f32",), [dense_item(2, 256)], (4, LIN), (4, LIN)),
    ("d_hw35", ("f32",), [dense_item(2, 35)], (1, TILED), (1, TILED)),
    # e, f, g. the corpus
    ("corpus", ("f32",), [dense_item(8, 256)], (4, LIN), (4, LIN)),
    ("corpus", ("bf16",), [dense_item(8, 256)], (4, LIN), (4, LIN)),
]
FORMS = {(name, dt): (fwd, bwd) for name, dts, _, fwd, bwd in CASES for dt in dts}
