"""The checkerboard context convolution (include/flashgmm_amd.h section 5b, flashgmm_amd/csrc/fgmm_ckbd_ctx.hip) restated in numpy:
the tap list, the neighbour map, the gather, and from them the reference every layer is held to.

  TAPS                      the 12 kernel positions (i, j) of the 5x5 with i + j odd, row-major
  neighbours(h, w, parity)  [12, h * w/2]: the compact anchor index tap t of the non-anchor at compact position q reads, -1 = outside
  gather(A, parity)         X [12 M, h * w/2]: X[t M + c][q] = A[c][neighbour] or +0 outside the image
  pack(W)                   Wk [C_out, 12 M]: Wk[o][t M + c] = W[o][c][tap t]
  chain(W, b, A, parity)    oracle.head_params(Wk, b, X): THE definition - acc = b[o]; t ascending, c ascending: acc = fmaf(w, x, acc)
  exact(W, b, A, parity)    the same sum in float64 (tests/head_ref.py)
  bound(W, b, A, parity)    head_ref.chain_bound with c_in = 12 M: how far the chain may be from the float64 sum
  CORPUS                    the smallest shapes at which the kernel can still go wrong

The positions are the reference's (compressai/latent_codecs/checkerboard.py:341-352), restated: with s = 0 for anchor_parity "even"
and 1 for "odd", the anchor at compact (r, j) is full-size (r, 2 j + ((r + s) & 1)), the non-anchor (r, 2 j + 1 - ((r + s) & 1))."""
from __future__ import annotations

import numpy as np

from tests import head_ref as H

F32 = np.float32
TAPS = [(i, j) for i in range(5) for j in range(5) if (i + j) & 1]
PARITIES = ("even", "odd")

# (h, w, M, C_out, N).  (1, 2): a single output, every vertical tap outside; (5, 6): every tap inside somewhere; (9, 30): 135 compact
# positions - past a wave's 32 and a block's 128.  M = 1, 2, 31, 32, 33, 65: the edges of the 32-channel K tile; C_out = 1, 31, 32, 33,
# 193: the edges of the 32-row tile and the 192-row group; N = 1, 3.
CORPUS = [
    (1, 2, 1, 1, 1),
    (2, 2, 2, 31, 3),
    (3, 4, 31, 32, 1),
    (5, 6, 32, 33, 1),
    (9, 30, 33, 193, 1),
    (9, 30, 65, 33, 3),
    (5, 6, 65, 193, 1),
    (1, 2, 33, 32, 1),
]


def shift(parity: str) -> int:
    return {"even": 0, "odd": 1}[parity]


def anchor_cols(h: int, w: int, parity: str) -> np.ndarray:
    """[h, w/2]: the full-size column of the anchor at compact (r, j)"""
    r, j = np.mgrid[0:h, 0:w // 2]
    return 2 * j + ((r + shift(parity)) & 1)


def non_anchor_cols(h: int, w: int, parity: str) -> np.ndarray:
    """[h, w/2]: the full-size column of the non-anchor at compact (r, j)"""
    r, j = np.mgrid[0:h, 0:w // 2]
    return 2 * j + 1 - ((r + shift(parity)) & 1)


def neighbours(h: int, w: int, parity: str) -> np.ndarray:
    """[12, h * w/2] int64: for tap t and the non-anchor at compact position q = r * w/2 + j, the compact index of the anchor it reads,
    -1 where the tap falls outside the image.  (Inside, the position is an anchor: asserted.)"""
    assert w % 2 == 0 and w >= 2 and h >= 1
    w2 = w // 2
    rows = np.mgrid[0:h, 0:w2][0]
    cols = non_anchor_cols(h, w, parity)
    is_anchor = np.zeros((h, w), bool)
    is_anchor[rows, anchor_cols(h, w, parity)] = True
    out = np.full((len(TAPS), h * w2), -1, np.int64)
    for t, (i, j) in enumerate(TAPS):
        rr, cc = rows + i - 2, cols + j - 2
        inside = (rr >= 0) & (rr < h) & (cc >= 0) & (cc < w)
        assert is_anchor[rr[inside], cc[inside]].all()
        idx = np.where(inside, rr * w2 + cc // 2, -1)
        out[t] = idx.reshape(-1)
    return out


def gather(A: np.ndarray, parity: str) -> np.ndarray:
    """A [M, h, w/2] float32 -> X [12 M, h * w/2]: row t M + c holds, for every compact non-anchor position, what tap t reads of
    channel c (+0.0 outside the image)"""
    M, h, w2 = A.shape
    nb = neighbours(h, 2 * w2, parity)
    flat = np.ascontiguousarray(A, F32).reshape(M, h * w2)
    X = np.zeros((len(TAPS), M, h * w2), F32)
    for t in range(len(TAPS)):
        ok = nb[t] >= 0
        X[t][:, ok] = flat[:, nb[t][ok]]
    return X.reshape(len(TAPS) * M, h * w2)


def pack(W: np.ndarray) -> np.ndarray:
    """W [C_out, M, 5, 5] -> Wk [C_out, 12 M], Wk[o][t M + c] = W[o][c][tap t]"""
    W = np.asarray(W, F32)
    return np.ascontiguousarray(np.stack([W[:, :, i, j] for i, j in TAPS], 1).reshape(W.shape[0], -1))


def chain(W, b, A, parity: str) -> np.ndarray:
    """the definition: [C_out, h, w/2] float32, bit for bit what the operator must give for one item A [M, h, w/2]"""
    from oracle import oracle as O

    _, h, w2 = A.shape
    return O.head_params(pack(W), b, gather(A, parity)).reshape(W.shape[0], h, w2)


def exact(W, b, A, parity: str) -> np.ndarray:
    _, h, w2 = A.shape
    return H.exact(pack(W), b, gather(A, parity)).reshape(W.shape[0], h, w2)


def bound(W, b, A, parity: str) -> np.ndarray:
    _, h, w2 = A.shape
    return H.chain_bound(pack(W), b, gather(A, parity)).reshape(W.shape[0], h, w2)


def masked(W: np.ndarray) -> np.ndarray:
    """W with its 13 dropped taps (i + j even) set to +0: the effective weight of a checkerboard-masked convolution"""
    out = np.zeros_like(W)
    for i, j in TAPS:
        out[:, :, i, j] = W[:, :, i, j]
    return out


def make_case(seed: int, h: int, w: int, M: int, C_out: int, N: int):
    """-> (W [C_out, M, 5, 5] masked, b [C_out], A [N, M, h, w/2]), float32, values of order one"""
    rng = np.random.default_rng(seed)
    W = masked((rng.standard_normal((C_out, M, 5, 5)) / np.sqrt(12 * M)).astype(F32))
    b = rng.standard_normal(C_out).astype(F32)
    A = np.round(rng.standard_normal((N, M, h, w // 2)) * 4).astype(F32)  # decoded latents are integers; some are 0
    A += (rng.standard_normal(A.shape) * (rng.random(A.shape) < 0.5)).astype(F32)  # ... and some are not (a weighted-mean quantizer)
    return W, b, A.astype(F32)
