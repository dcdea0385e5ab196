"""The bf16x6 hidden layer's bound (header section 2c): head_ref's bf16x6 derivation with n16 = ceil(c_a / 16) + ceil(c_b / 16), through the activation."""
import numpy as np

from tests import head_ref as H
from tests.test_gpu_param_body import act_ref


def bound(W, b, xa, xb, act, slope):  # -> (want, bound) [c_out, hw] float64, for one item xa [c_a, hw] or None (absent), xb [c_b, hw]
    c_a = W.shape[1] - xb.shape[0]
    (Wc, x, n16) = (W[:, c_a:], xb, -(-xb.shape[0] // 16)) if xa is None else (W, np.concatenate([xa, xb]), -(-c_a // 16) - (-xb.shape[0] // 16))
    rel, a0 = H.bf16x6_terms(16 * n16)
    s, want = H.abs_sum(Wc, b, x), act_ref(H.exact(Wc, b, x), act, slope)
    l1, lx = np.abs(Wc.astype(np.float64)).sum(1)[:, None], np.abs(x.astype(np.float64)).sum(0)[None, :]
    return want, max(1.0, abs(slope)) * (rel * s + H.BF16_SUB * (l1 + lx) + a0 + Wc.shape[1] * 2.0**-52 * s) + 2.0**-24 * np.abs(want) + 2.0**-150
