"""The arithmetic of include/flashgmm_amd.h section 3j - the entropy bottleneck's forward(): the factorized density at both edges of an
element's bin, the mirrored difference of sigmoids, the bound - in a few lines of torch, in binary32 or binary64, and the seeded corpus
the entropy-bottleneck tests share.

``forward`` follows the header operation by operation (sums from the left, separate multiply and add), so its float32 evaluation is the
kernel's arithmetic in torch operations; ``mirrored=False`` gives the reference's written form ``sig(up) - sig(lo)``.  Gradients come
from autograd through ``forward`` (``gradients``), with ``torch.sigmoid`` standing for ``1 / (1 + exp(-a))``: the same function, whose
backward stays finite where ``exp`` overflows in the branch ``torch.where`` does not select.  tests/test_entropy_bottleneck_cpu.py ties
the float64 evaluation of both to the reference's own class through tests/golden/g11_entropy_bottleneck.npz (written by
tests/golden/make_golden_eb.py).

The corpus: C = 6 channels, x ``[2, 6, 16, 16]``.  Parameters are the reference's initial values plus N(0, 0.5) on the matrices, biases
U(-0.5, 0.5), factors N(0, 0.7), medians U(-3, 3); planted on top: one matrix entry at 25 (softplus' linear branch) and one factor of 2
(|tanh| = 0.96).  Of every channel's elements half are N(0, 8) (the body), a quarter U(-400, -60) (the left tail) and a quarter
U(60, 400) (the right tail); the upstream gradient g has both signs in every region.
"""
import numpy as np
import torch

LB = 1e-9  # the reference's default likelihood bound; the kernel and the reference hold it as binary32
LN2F = float.fromhex("0x1.62e430p-1")
SEED = 20261020
C = 6
SHAPE = (2, C, 16, 16)
FILTERS = (3, 3, 3, 3)
NAMES = tuple(n for i in range(5) for n in ([f"_matrix{i}", f"_bias{i}"] + ([f"_factor{i}"] if i < 4 else [])))  # theta's order
SIZES = tuple(s for i in range(5) for s in ([9 if 0 < i < 4 else 3, 3 if i < 4 else 1] + ([3] if i < 4 else [])))
REGIONS = ("body", "left", "right")
PLANT_MATRIX = ("_matrix2", (1, 2, 0), 25.0)
PLANT_FACTOR = ("_factor1", (3, 1, 0), 2.0)
assert sum(SIZES) == 58 and len(NAMES) == 14


def f32(x):
    return float(np.float32(x))


def init_params(channels, init_scale=10.0, rng=None):
    """the reference's initial values (entropy_models.py:360-385) as float32 arrays; the biases from ``rng`` (U(-0.5, 0.5)) or zero"""
    width = (1,) + FILTERS + (1,)
    scale = init_scale ** (1 / (len(FILTERS) + 1))
    p = {}
    for i in range(len(FILTERS) + 1):
        p[f"_matrix{i}"] = np.full((channels, width[i + 1], width[i]), np.log(np.expm1(1 / scale / width[i + 1])), np.float32)
        p[f"_bias{i}"] = (rng.uniform(-0.5, 0.5, (channels, width[i + 1], 1)) if rng is not None else np.zeros((channels, width[i + 1], 1))).astype(np.float32)
        if i < len(FILTERS):
            p[f"_factor{i}"] = np.zeros((channels, width[i + 1], 1), np.float32)
    return p


def corpus(seed=SEED, shape=SHAPE):
    """-> (x [B, C, h, w], params {name: array}, med [C], g like x, region like x: 0 body, 1 left tail, 2 right tail), float32"""
    rng = np.random.default_rng(seed)
    B, Cn, h, w = shape
    p = init_params(Cn, rng=rng)
    for name in NAMES:
        if "matrix" in name:
            p[name] = (p[name] + rng.normal(0, 0.5, p[name].shape)).astype(np.float32)
        elif "factor" in name:
            p[name] = rng.normal(0, 0.7, p[name].shape).astype(np.float32)
    for name, at, value in (PLANT_MATRIX, PLANT_FACTOR):
        if at[0] < Cn:
            p[name][at] = value
    med = rng.uniform(-3, 3, Cn).astype(np.float32)
    region = rng.permutation(np.repeat(np.array([0, 0, 1, 2], np.int8), (B * Cn * h * w + 3) // 4)[: B * Cn * h * w]).reshape(shape)
    x = np.where(region == 0, rng.normal(0, 8, shape), np.where(region == 1, rng.uniform(-400, -60, shape), rng.uniform(60, 400, shape))).astype(np.float32)
    g = (rng.standard_normal(shape) * np.exp(rng.uniform(-2, 2, shape))).astype(np.float32)
    return x, p, med, g, region


def theta_of(params):
    """{name: [C, out, in]} (arrays or tensors) -> theta [C, 58] in the header's order"""
    parts = [torch.as_tensor(params[n]) for n in NAMES]
    return torch.cat([t.reshape(t.shape[0], -1) for t in parts], 1)


def split_theta(theta):
    """theta [C, 58] (array) -> {name: [C, out, in]}"""
    out, at = {}, 0
    for n, s in zip(NAMES, SIZES):
        rows = 1 if n.endswith("4") else 3
        out[n] = np.ascontiguousarray(theta[:, at:at + s]).reshape(theta.shape[0], rows, s // rows)
        at += s
    return out


def chain(P, x):
    """x [C, n] -> the cumulative logits [C, n]; P: {name: tensor [C, out, in]} of x's dtype"""
    H = torch.nn.functional.softplus(P["_matrix0"])  # torch's: m > 20 ? m : log1p(exp(m))
    a = H[:, :, 0:1] * x[:, None, :] + P["_bias0"]
    h = a + torch.tanh(P["_factor0"]) * torch.tanh(a)
    for i in range(1, 5):
        H = torch.nn.functional.softplus(P[f"_matrix{i}"])
        a = ((H[:, :, 0:1] * h[:, 0:1] + H[:, :, 1:2] * h[:, 1:2]) + H[:, :, 2:3] * h[:, 2:3]) + P[f"_bias{i}"]
        h = a + torch.tanh(P[f"_factor{i}"]) * torch.tanh(a) if i < 4 else a
    return h[:, 0]


def forward(x, params, med, mode, lb=LB, dtype=torch.float32, mirrored=True, sig=None):
    """x [B, C, ...], params {name: tensor}, med [C] -> dict of v, lo, up, flip, L and the bounded ``out``, shaped like x.  Inputs are
    converted to ``dtype`` exactly; the bound is the binary32 value of ``lb`` widened."""
    sig = sig or (lambda a: 1 / (1 + torch.exp(-a)))
    shape, Cn = x.shape, x.shape[1]
    P = {n: params[n].to(dtype) for n in NAMES}
    xc = x.to(dtype).reshape(shape[0], Cn, -1).permute(1, 0, 2).reshape(Cn, -1)
    m = med.to(dtype).reshape(Cn, 1)
    v = torch.round(xc - m) + m if mode else xc
    lo, up = chain(P, v - 0.5), chain(P, v + 0.5)
    flip = (lo + up) > 0
    L = torch.where(flip, sig(-lo) - sig(-up), sig(up) - sig(lo)) if mirrored else sig(up) - sig(lo)
    lbt = torch.tensor(f32(lb), dtype=dtype, device=x.device)
    out = torch.where((L > lbt) | torch.isnan(L), L, lbt) if lb > 0 else L
    back = lambda t: t.reshape(Cn, shape[0], -1).permute(1, 0, 2).reshape(shape)  # noqa: E731
    return {k: back(t) for k, t in dict(v=v, lo=lo, up=up, flip=flip, L=L, out=out).items()}


def gradients(x, params, med, g, mode, lb=LB, dtype=torch.float32, g_bits=None):
    """autograd through ``forward`` with the header's pass-through rule -> {"x", the 14 names, "med"}: the gradients of sum(out * g), or
    (``g_bits`` [B]) of sum_b g_bits[b] * bits[b], bits[b] = sum(-log2(out)) over item b's elements with a finite out > 0.  The
    gradient of x is zero with ``mode``; that of med is zero without."""
    leaves = {n: params[n].detach().to(dtype).requires_grad_(True) for n in NAMES}
    xl, ml = x.detach().to(dtype).requires_grad_(True), med.detach().to(dtype).requires_grad_(True)
    f = forward(xl, leaves, ml, mode, lb, dtype, sig=torch.sigmoid)
    L, out = f["L"], f["out"].detach()
    if g_bits is not None:
        counts = (out > 0) & (out < float("inf"))
        gb = torch.as_tensor(g_bits).to(device=x.device, dtype=torch.float32).reshape(-1, *([1] * (x.dim() - 1))).to(dtype)
        g = torch.where(counts, -gb / (out * torch.tensor(LN2F, dtype=dtype, device=x.device)), torch.zeros_like(out))
    else:
        g = g.to(dtype)
    lbt = f32(lb)
    gL = torch.where((L.detach() >= lbt) | (g < 0) | (lbt <= 0), g, torch.zeros_like(g))  # the select of the header
    (L * gL).sum().backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    return {"x": zero(xl), "med": zero(ml), **{n: zero(leaves[n]) for n in NAMES}}


def bits_of(out, dtype=np.float64):
    """host sum of the header's rate: out [B, ...] (array) -> (bits_q int64 [B], n_nonfinite int64 [B])"""
    o = out.reshape(out.shape[0], -1).astype(np.float64)
    counts = (o > 0) & np.isfinite(o)
    q = np.rint(-np.log2(np.where(counts, o, 1.0)) * 2.0 ** 32).astype(np.int64)
    return np.where(counts, q, 0).sum(1), (~counts).sum(1)
