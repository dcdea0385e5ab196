"""The dense 3x3 / 5x5 convolution layer of header section 5d restated in numpy: the definition the HIP kernel (fgmm_conv.hip) is held to.

  im2col(x, k)     [c, h, w] -> X [c k^2, h w]: row c k^2 + t is tap t = a k + b of channel c, +0 outside the image
  chain(...)       oracle.head_params' fmaf chain over W.reshape(c_out, c_in k^2) and X, the activation in float32, the shuffle
  exact, bound     the same sum in float64 and the chain's error bound (tests/head_ref.py, with c_in k^2 terms)
  CASES            (k, h, w, c_in, c_out, n, shuffle, act) at the edges of the kernel's constants: 8 x 16 patch, chunks of 8 channels,
                   row tiles of 32, the tallest block of 4 row tiles
"""
import numpy as np

from tests import head_ref as H

F32 = np.float32
NONE, LEAKY, RELU = 0, 1, 2  # FGMM_ACT_*
T_MAX = 4

CASES = [(3, 1, 1, 1, 1, 1, 1, NONE), (5, 2, 3, 2, 31, 3, 1, RELU), (5, 8, 16, 8, 32, 1, 1, LEAKY), (3, 9, 17, 9, 33, 1, 1, LEAKY),
         (5, 17, 33, 17, 65, 2, 1, RELU), (3, 8, 16, 16, 128, 1, 2, LEAKY), (3, 3, 5, 7, 36, 2, 2, NONE), (5, 5, 6, 33, 32 * T_MAX + 1, 1, 1, NONE)]


def im2col(x, k):
    c, h, w = x.shape
    xp = np.zeros((c, h + k - 1, w + k - 1), F32)
    xp[:, k // 2:k // 2 + h, k // 2:k // 2 + w] = x
    return np.stack([xp[:, a:a + h, b:b + w] for a in range(k) for b in range(k)], 1).reshape(c * k * k, h * w)


def act_ref(v, act, slope):
    with np.errstate(all="ignore"):
        if act == LEAKY:
            return np.where(v > 0, v, v * v.dtype.type(F32(slope)))  # (the layer's slope is the binary32 number)
        return np.where(v > 0, v, np.where(np.isnan(v), v, np.zeros_like(v))) if act == RELU else v


def shuffled(v, shuffle):
    """[c, h, w] -> PixelShuffle(shuffle) of it"""
    c, h, w = v.shape
    s = shuffle
    return v.reshape(c // (s * s), s, s, h, w).transpose(0, 3, 1, 4, 2).reshape(c // (s * s), h * s, w * s)


def chain(oracle, W, b, x, act=NONE, slope=0.0, shuffle=1):
    """W [c_out, c_in, k, k], b [c_out] or None, x [n, c_in, h, w] -> the layer's output, float32"""
    k, (n, _, h, w) = W.shape[-1], x.shape
    return np.stack([shuffled(act_ref(oracle.head_params(W.reshape(W.shape[0], -1), b, im2col(xi, k)), act, slope).reshape(-1, h, w), shuffle) for xi in x])


def exact(W, b, xi):
    return H.exact(W.reshape(W.shape[0], -1), b, im2col(xi, W.shape[-1]))


def bound(W, b, xi):
    return H.chain_bound(W.reshape(W.shape[0], -1), b, im2col(xi, W.shape[-1]))


def make(seed, k, h, w, c_in, c_out, n, bias=True):
    r = np.random.default_rng(seed)
    g = lambda *s: r.standard_normal(s).astype(F32)
    return g(c_out, c_in, k, k), g(c_out) if bias else None, g(n, c_in, h, w)
