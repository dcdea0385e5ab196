"""The gradients of the dense 3x3 / 5x5 layer (header section 5f) restated in numpy over tests/conv_ref.py: gz by section 2d's rule through
the un-shuffle; the data gradient as conv_ref.chain on the flipped, transposed weight; the slice rule and the order of the positions; the
weight gradient per slice as oracle.head_params with the roles exchanged, then binary32 adds; the float64 sums and their bounds."""
import numpy as np
import torch

from tests import conv_ref as R
from tests import head_ref as H

F32 = np.float32
SLICE_MIN, SLICES_MAX = 256, 16  # FGMM_CONV_WGRAD_SLICE_MIN / FGMM_CONV_WGRAD_SLICES_MAX, restated


def gz(gy, out, act, slope, shuffle=1):  # [n, c / s^2, h s, w s] x 2 -> the pre-activation's gradient [n, c, h, w] (conv_ref.shuffled, inverted)
    s, (n, c, hs, ws) = shuffle, gy.shape
    g, o = (v.reshape(n, c, hs // s, s, ws // s, s).transpose(0, 1, 3, 5, 2, 4).reshape(n, c * s * s, hs // s, ws // s) for v in (gy, out))
    with np.errstate(all="ignore"):
        return g if act == R.NONE else np.where(o > 0, g, g * F32(slope) if act == R.LEAKY else F32(0)).astype(F32)


flip_transpose = lambda W: np.ascontiguousarray(W.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])
data_grad = lambda oracle, W, g: R.chain(oracle, flip_transpose(W), None, g)


def slices(n, h, w):
    nb = n * -(-h // 8)
    B = -(-nb // min(SLICES_MAX, -(-n * h * w // SLICE_MIN), nb))
    return -(-nb // B), B


def positions(n, h, w):
    """per slice: flat indices i * h * w + r * w + q, in the header's order (items, bands of 8 rows, patches of 16 columns, row-major)"""
    S, B = slices(n, h, w)
    bands = [[(i * h + r) * w + q for q0 in range(0, w, 16) for r in range(r0, min(r0 + 8, h)) for q in range(q0, min(q0 + 16, w))]
             for i in range(n) for r0 in range(0, h, 8)]
    return [np.array(sum(bands[j * B:(j + 1) * B], []), np.int64) for j in range(S)]


def weight_grad(oracle, x, g, k, rows=slice(None)):  # -> (dW, dbias); rows: the output channels asked for (a chain reads its own channel's gz alone)
    (n, c_in, h, w), G = x.shape, np.ascontiguousarray(g[:, rows].transpose(1, 0, 2, 3).reshape(-1, x.shape[0] * x.shape[2] * x.shape[3]))
    X = np.concatenate([np.concatenate([R.im2col(xi, k) for xi in x], 1), np.ones((1, G.shape[1]), F32)])  # the forward's taps, then the bias' ones
    acc = None
    for at in positions(n, h, w):
        part = oracle.head_params(np.ascontiguousarray(G[:, at]), None, np.ascontiguousarray(X[:, at].T))  # acc = +0; s ascending: fmaf(gz, x, acc)
        with np.errstate(invalid="ignore"):
            acc = part if acc is None else (acc + part).astype(F32)
    return acc[:, :-1].reshape(-1, c_in, k, k), acc[:, -1]


def exact(x, W, g, extra=0):
    """-> the float64 sums (dx, dW, dbias) and their bounds: head_ref.chain_bound's form with the gradient's depth d - c_out k^2 terms for dx; for dW, dbias a slice's
    L positions and S - 1 adds, depth L + S - 1 at the most; `extra`: roundings already in the terms (gy * slope: 1) - times the sum of |terms|, the magnitudes' gradient"""
    (n, _, h, w), k = x.shape, W.shape[-1]

    def sums(f):
        t = [torch.from_numpy(f(v)).double().requires_grad_(True) for v in (x, W, np.zeros(len(W), F32))]
        return [v.numpy() for v in torch.autograd.grad(torch.nn.functional.conv2d(*t, padding=k // 2), t, torch.from_numpy(f(g)).double())]

    d_w = max(len(at) for at in positions(n, h, w)) + slices(n, h, w)[0] - 1 + extra
    return sums(np.asarray), [(H.gamma(d) + d * 2.0**-52) * m + d * H.ETA for d, m in zip((len(W) * k * k + extra, d_w, d_w), sums(np.abs))]
