"""The gradients of the checkerboard context convolution (include/flashgmm_amd.h section 5c, flashgmm_amd/csrc/fgmm_ckbd_ctx_grad.hip)
restated in numpy over tests/ckbd_ctx_ref.py - the reference every layer is held to.

  slices(P)                     (S, L): the weight gradient's slice rule, a function of P = n_items * h * w/2 alone
  slice_ranges(P)               the S half-open ranges [k L, min((k + 1) L, P))
  flip_transpose(W)             W'[c][o][i][j] = W[o][c][4 - i][4 - j]
  data_grad(W, g, parity)       dA [M, h, w/2] of ONE item: ckbd_ctx_ref.chain on W' with the other parity - THE definition
  weight_grad(A, g, parity)     (dW [C_out, M, 5, 5], dbias [C_out]) over ALL items: per slice oracle.head_params with the roles exchanged
                                (g as the weights, the gathered features transposed), then binary32 adds ascending - THE definition
  *_exact, *_abs                the same sums, and the sums of the absolute terms, in float64
  CORPUS                        ckbd_ctx_ref.CORPUS and the shapes at which the slicing can go wrong"""
from __future__ import annotations

import numpy as np

from tests import ckbd_ctx_ref as R
from tests import head_ref as H

F32 = np.float32
SLICE_MIN, SLICES_MAX = 256, 16  # the header's FGMM_CKBD_WGRAD_SLICE_MIN / FGMM_CKBD_WGRAD_SLICES_MAX, restated

# (h, w, M, C_out, N): (9, 30, 2, 3, 3) is P = 405 - two slices, both item boundaries (135, 270) inside a slice; (16, 32, 2, 3, 17) is
# P = 4352 - the cap of 16 slices, the last one 32 long; (1, 2, 1, 1, 1), P = 1, is ckbd_ctx_ref.CORPUS' first
CORPUS = list(R.CORPUS) + [(9, 30, 2, 3, 3), (16, 32, 2, 3, 17)]
assert (1, 2, 1, 1, 1) in CORPUS


def slices(P: int):
    s0 = min(SLICES_MAX, -(-P // SLICE_MIN))
    L = 32 * -(-P // (32 * s0))
    return -(-P // L), L


def slice_ranges(P: int):
    S, L = slices(P)
    return [(k * L, min((k + 1) * L, P)) for k in range(S)]


def other(parity: str) -> str:
    return {"even": "odd", "odd": "even"}[parity]


def flip_transpose(W: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(W, F32).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def data_grad(W, g, parity: str) -> np.ndarray:
    """g [C_out, h, w/2], the gradient at one item's non-anchors -> dA [M, h, w/2] at its anchors"""
    return R.chain(flip_transpose(W), None, g, other(parity))


def data_grad_exact(W, g, parity: str) -> np.ndarray:
    return R.exact(flip_transpose(W), None, g, other(parity))


def data_grad_abs(W, g, parity: str) -> np.ndarray:
    Wt = flip_transpose(W)
    return H.abs_sum(R.pack(Wt), None, R.gather(g, other(parity))).reshape((Wt.shape[0],) + g.shape[1:])


def features(A, parity: str) -> np.ndarray:
    """A [N, M, h, w/2] -> X [12 M, P]: the gathered features of all items, concatenated along the positions"""
    return np.ascontiguousarray(np.concatenate([R.gather(a, parity) for a in A], axis=1))


def rows(g) -> np.ndarray:
    """g [N, C_out, h, w/2] -> G [C_out, P]"""
    g = np.asarray(g, F32)
    return np.ascontiguousarray(g.transpose(1, 0, 2, 3).reshape(g.shape[1], -1))


def scatter(cols: np.ndarray, M: int) -> np.ndarray:
    """[C_out, 12 M] (column t M + c) -> [C_out, M, 5, 5], +0 at the dropped taps"""
    out = np.zeros((cols.shape[0], M, 5, 5), cols.dtype)
    for t, (i, j) in enumerate(R.TAPS):
        out[:, :, i, j] = cols[:, t * M:(t + 1) * M]
    return out


def weight_grad(A, g, parity: str):
    from oracle import oracle as O

    X, G = features(A, parity), rows(g)
    M = A.shape[1]
    dw = db = None
    for k, (s0, s1) in enumerate(slice_ranges(G.shape[1])):
        Gk = G[:, s0:s1]
        pw = O.head_params(Gk, None, np.ascontiguousarray(X[:, s0:s1].T))  # [C_out, 12 M]: acc = +0; s ascending: fmaf(g, x, acc)
        pb = O.head_params(Gk, None, np.ones((s1 - s0, 1), F32))[:, 0]
        with np.errstate(invalid="ignore"):  # (inf - inf among the partials is a NaN the kernel gives as well)
            dw, db = (pw, pb) if k == 0 else ((dw + pw).astype(F32), (db + pb).astype(F32))
    return scatter(dw, M), db


def weight_grad_exact(A, g, parity: str):
    X, G = features(A, parity).astype(np.float64), rows(g).astype(np.float64)
    return scatter(G @ X.T, A.shape[1]), G.sum(1)


def weight_grad_abs(A, g, parity: str):
    X, G = np.abs(features(A, parity).astype(np.float64)), np.abs(rows(g).astype(np.float64))
    return scatter(G @ X.T, A.shape[1]), G.sum(1)


def make_case(seed: int, h: int, w: int, M: int, C_out: int, N: int):
    """-> (W masked, b, A [N, M, h, w/2], g [N, C_out, h, w/2]) float32: ckbd_ctx_ref.make_case and an output gradient of order one"""
    W, b, A = R.make_case(seed, h, w, M, C_out, N)
    g = np.random.default_rng(seed + 7919).standard_normal((N, C_out, h, w // 2)).astype(F32)
    return W, b, A, g
