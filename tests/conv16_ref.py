"""The bf16x6 dense convolution's bound (header section 5d, FGMM_CONV_BF16X6): tests/head_ref.py's bf16x6 derivation over the problem
W.reshape(c_out, c_in k^2), im2col(x) of tests/conv_ref.py with n16 = k^2 ceil(c_in / 16) - a channel tile is padded for every tap, so not
ceil(c_in k^2 / 16) - through the activation, as tests/hidden16_ref.py carries its own."""
import numpy as np

from tests import conv_ref as R
from tests import head_ref as H


def bound(W, b, xi, act, slope):  # -> (want, bound) [c_out, h w] float64, for one item xi [c_in, h, w]
    k = W.shape[-1]
    Wk, X = W.reshape(W.shape[0], -1), R.im2col(xi, k)
    rel, a0 = H.bf16x6_terms(16 * k * k * -(-W.shape[1] // 16))
    s, want = H.abs_sum(Wk, b, X), R.act_ref(R.exact(W, b, xi), act, slope)
    l1, lx = np.abs(Wk.astype(np.float64)).sum(1)[:, None], np.abs(X.astype(np.float64)).sum(0)[None, :]
    return want, max(1.0, abs(slope)) * (rel * s + H.BF16_SUB * (l1 + lx) + a0 + Wk.shape[1] * 2.0**-52 * s) + 2.0**-24 * np.abs(want) + 2.0**-150
