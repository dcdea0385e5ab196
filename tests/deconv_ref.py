"""The transposed 3x3 / 5x5 convolution layer of header section 5e (stride 1 | 2, padding k // 2, output padding stride - 1) restated in
numpy: the definition the HIP kernels (fgmm_deconv.hip; fgmm_conv.hip over the flipped pack) are held to.  One output phase is a dense
product - its weights in chain order [c_out, c_in nt] times the im2col of its nt kept taps, +0 outside the image, a tap with an odd u or v
no row at all - run through oracle.head_params' fmaf chain (chain), in float64 (exact) and bounded by tests/head_ref.py with the
phase's c_in nt terms (bound).  CASES: (k, s, h, w, c_in, c_out, n, act) at the kernel's constants: 8 x 16 patch, chunks of 8, row tiles of 32."""
import numpy as np

from tests import head_ref as H
from tests.conv_ref import F32, LEAKY, NONE, RELU, act_ref

CASES = [(5, 2, 1, 1, 1, 1, 1, NONE), (3, 2, 1, 1, 1, 1, 1, NONE), (5, 2, 8, 16, 8, 32, 1, LEAKY), (5, 2, 9, 17, 9, 33, 2, RELU), (3, 2, 9, 17, 9, 33, 1, LEAKY),
         (5, 2, 3, 5, 17, 65, 1, NONE), (3, 1, 9, 17, 9, 33, 1, NONE), (5, 1, 5, 6, 17, 65, 2, RELU)]


def taps(k, s, par):  # the kept taps a' of output parity par along one axis, each with the input offset it reads
    return [(a, (par + a - k // 2) // s) for a in range(k) if (par + a - k // 2) % s == 0]


def phase(W, xi, s, pr, pc):
    """W [c_in, c_out, k, k], xi [c_in, h, w] -> (Wp, X) of outputs (s r + pr, s q + pc): K index c nt + (kept tap row, kept tap column)"""
    k, (c, h, w) = W.shape[-1], xi.shape
    ta, tb = taps(k, s, pr), taps(k, s, pc)
    xp = np.zeros((c, h + 4, w + 4), F32)
    xp[:, 2:2 + h, 2:2 + w] = xi
    X = np.stack([xp[:, 2 + dr:2 + dr + h, 2 + dc:2 + dc + w] for _, dr in ta for _, dc in tb], 1).reshape(-1, h * w)
    Wp = np.stack([W[:, :, k - 1 - a, k - 1 - b].T for a, _ in ta for b, _ in tb], 2).reshape(W.shape[1], -1)
    return np.ascontiguousarray(Wp), np.ascontiguousarray(X)


def per_phase(fn, W, b, xi, s):
    """fn(Wp, b, X) -> [c_out, h w] of every phase, interleaved into [c_out, s h, s w]"""
    _, h, w = xi.shape
    out = None
    for pr in range(s):
        for pc in range(s):
            Wp, X = phase(W, xi, s, pr, pc)
            v = fn(Wp, b, X)
            out = np.empty((W.shape[1], s * h, s * w), v.dtype) if out is None else out
            out[:, pr::s, pc::s] = v.reshape(-1, h, w)
    return out


def chain(oracle, W, b, x, s, act=NONE, slope=0.0):
    """W [c_in, c_out, k, k], b [c_out] or None, x [n, c_in, h, w] -> the layer's output [n, c_out, s h, s w], float32"""
    return np.stack([act_ref(per_phase(oracle.head_params, W, b, xi, s), act, slope) for xi in x])


exact = lambda W, b, xi, s: per_phase(H.exact, W, b, xi, s)
bound = lambda W, b, xi, s: per_phase(H.chain_bound, W, b, xi, s)


def make(seed, k, h, w, c_in, c_out, n, bias=True):
    r = np.random.default_rng(seed)
    g = lambda *sh: r.standard_normal(sh).astype(F32)
    return g(c_in, c_out, k, k), g(c_out) if bias else None, g(n, c_in, h, w)
