"""The bf16x6 context convolution's bound (header section 5b, FGMM_CKBD_CTX_BF16X6): tests/head_ref.py's bf16x6 derivation over the gathered
problem of tests/ckbd_ctx_ref.py with n16 = 12 ceil(M / 16) - a tap's last tile is padded, so not ceil(12 M / 16)."""
import numpy as np

from tests import ckbd_ctx_ref as R
from tests import head_ref as H

CORPUS = R.CORPUS + [(5, 6, M, 33, 1) for M in (15, 16, 17)]  # + the edges of the 16-channel K tile


def bound(W, b, A, parity):  # -> [C_out, h, w/2] float64, for one item A [M, h, w/2]
    Wk, X = R.pack(W), R.gather(A, parity)
    rel, a0 = H.bf16x6_terms(16 * 12 * -(-W.shape[1] // 16))
    s = H.abs_sum(Wk, b, X)
    l1, lx = np.abs(Wk.astype(np.float64)).sum(1)[:, None], np.abs(X.astype(np.float64)).sum(0)[None, :]
    return (rel * s + H.BF16_SUB * (l1 + lx) + a0 + Wk.shape[1] * 2.0**-52 * s).reshape(W.shape[0], *A.shape[1:])
