"""The parameter head's last layer restated in float64, and the error bounds of its two arithmetics (tests/test_head_reference_cpu.py
derives and checks them on the CPU; tests/test_gpu_head_edges.py holds the HIP kernels to them).

  exact(W, b, x)          b + W x in float64: every binary32 product is exact there, the float64 sum is within c_in 2^-53 of exact
  chain_bound(...)        the fmaf chain (oracle.head_params, fgmm_head.hip): gamma_c_in (sum |w x| + |b|) + c_in 2^-150
  split3(v)               fgmm_head16.hip's split of a binary32 into three bfloat16 parts (round to nearest even at each step)
  bf16x6_bound(...)       fgmm_head16.hip: relative and absolute terms, derived below
  identity_head(M)        weights and bias of a head whose 12 M output planes are its 12 M input planes
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U = 2.0**-24        # unit roundoff of binary32
ETA = 2.0**-150     # the largest error of one rounding below the binary32 normal range (half the subnormal spacing)
BF16_SUB = 2.0**-133  # the spacing of the bfloat16 subnormals (7 stored bits below 2^-126)


def exact(W, b, x):
    """b + W x in float64 (IEEE: 0 * inf is NaN, inf - inf is NaN) -> [n_out, hw]"""
    with np.errstate(all="ignore"):
        if np.isfinite(W).all() and np.isfinite(x).all():
            out = W.astype(np.float64) @ x.astype(np.float64)
        else:  # a BLAS may pad with 0 * inf: the IEEE sum one input channel at a time
            out = _ieee_sum(W, x)
        if b is not None:
            out = out + b.astype(np.float64)[:, None]
    return out


def _ieee_sum(W, x):
    """sum_k w[o,k] x[k,p] in float64 with IEEE specials, one k at a time (small shapes: the non-finite families)"""
    Wd, xd = W.astype(np.float64), x.astype(np.float64)
    out = np.zeros((W.shape[0], x.shape[1]))
    with np.errstate(all="ignore"):
        for k in range(W.shape[1]):
            out = out + Wd[:, k:k + 1] * xd[k:k + 1, :]
    return out


def abs_sum(W, b, x):
    """sum_k |w x| + |b| in float64 (the scale every bound is relative to)"""
    with np.errstate(all="ignore"):
        s = np.abs(W.astype(np.float64)) @ np.abs(x.astype(np.float64))
        return s + (0.0 if b is None else np.abs(b.astype(np.float64))[:, None])


def gamma(n):
    return n * U / (1 - n * U)


def chain_bound(W, b, x):
    """|fmaf chain - exact| <= gamma_c_in (sum |w x| + |b|) + c_in 2^-150: c_in roundings, each at most u |partial sum| or, below
    the normal range, 2^-150; every partial sum is at most sum |w x| + |b|.  (+ the float64 reference's own c_in 2^-53.)"""
    c_in = W.shape[1]
    return (gamma(c_in) + c_in * 2.0**-52) * abs_sum(W, b, x) + c_in * ETA


def ieee_class(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a, np.float64)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


# ---- bfloat16 ---------------------------------------------------------------------------------------------------------
def to_bf16(v):
    """binary32 -> bfloat16 (as binary32 values) rounded to nearest even, as v_cvt_pk_bf16_f32: the subnormals on their 2^-133 grid,
    overflow to +-inf, NaN stays NaN"""
    v = np.ascontiguousarray(v, F32)
    u = v.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)
    return np.where(np.isnan(v), v, r).astype(F32)


def split3(v):
    """fgmm_head16.hip split3: v1 = bf16(v), v2 = bf16(v - v1), v3 = bf16(v - v1 - v2) (the subtractions in binary32)"""
    v = np.asarray(v, F32)
    with np.errstate(all="ignore"):
        a = to_bf16(v)
        r1 = (v - a).astype(F32)
        b = to_bf16(r1)
        r2 = (r1 - b).astype(F32)
        c = to_bf16(r2)
    return a, b, c


# The bf16x6 form computes b + sum_k of the six part products (w1 x3, w3 x1, w2 x2, w1 x2, w2 x1, w1 x1), one
# v_mfma_f32_32x32x16_bf16 per part product and 16 input channels, accumulated in binary32.  For finite w, x with |v| < 0x1.FFp127:
#   split:   |v - v1 - v2 - v3| = 0 while v3 is a normal bfloat16 (it then holds the last 8 bits of v exactly), and <= 2^-134 below
#            (v3 rounded to the subnormal grid); |v2| <= 2^-8 (1 + 2^-8) |v|, |v3| <= 2^-16 (1 + 2^-7) |v|
#   dropped: |w2 x3 + w3 x2 + w3 x3| <= 2^-23 (1 + 2^-6) |w x|
#   split residuals: |w x - (w1+w2+w3)(x1+x2+x3)| <= 2^-133 (|w| + |x|) (products of the two residuals are far below)
#   products: a bfloat16 product is exact in binary32 (16 significant bits) down to 2^-149; each of the 6 ceil(c_in / 16)
#            matrix steps rounds the accumulator once: <= u |partial| + 2^-150, |partial| <= (1 + 2^-7) (sum |w x| + |b|)
# so  |got - exact| <= R (sum |w x| + |b|) + A,   R = 2^-23 (1 + 2^-6) + 6 n16 u (1 + 2^-7),
#                                                 A = 2^-133 sum_k (|w_k| + |x_k|) + 6 n16 2^-150
# (the one-rounding-per-step model is the matrix core's; the GPU tests check it at c_in = 1 .. 1040).
def bf16x6_terms(c_in):
    n16 = -(-c_in // 16)
    return 2.0**-23 * (1 + 2.0**-6) + 6 * n16 * U * (1 + 2.0**-7), 6 * n16 * ETA


def bf16x6_bound(W, b, x):
    R, A0 = bf16x6_terms(W.shape[1])
    with np.errstate(all="ignore"):
        l1 = np.abs(W.astype(np.float64)).sum(1)[:, None]  # sum_k |w|
        lx = np.abs(x.astype(np.float64)).sum(0)[None, :]  # sum_k |x|
    return R * abs_sum(W, b, x) + BF16_SUB * (l1 + lx) + A0 + W.shape[1] * 2.0**-52 * abs_sum(W, b, x)


def bf16x6_features_in_domain(x):
    """the features the bf16x6 kernels take: every bfloat16 part finite (|x| < 0x1.FFp127, no NaN / inf)"""
    return bool(np.isfinite(to_bf16(x)).all())


# ---- a head that reproduces its input ---------------------------------------------------------------------------------
def identity_head(M):
    """W = I [12 M, 12 M], no bias: output plane o = input plane o, through one fmaf with +-0 partners - bit for bit, except that a
    -0 input comes out +0 when the chain starts at the +0 of no bias (and the identity row's zeros multiply other planes' -0s)"""
    return np.eye(12 * M, dtype=F32), None
