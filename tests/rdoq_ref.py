"""Shared by tests/test_rdoq_cpu.py and tests/test_gpu_rdoq.py: the reference side of rate-distortion optimised quantisation
(include/flashgmm_amd.h section 3c), numpy only.

For the symbols ``sym - 1, sym, sym + 1`` of every latent of a coded channel the oracle's table (``oracle.symtab``) is priced entry by
entry with the library's HOST function ``fgmm_symtab_bits`` (tests/rate_ref.py host_bits); the objective
``J(v) = d * d + lam_q * cost_q(v)``, ``d = float64(y) - float64(v)``, ``lam_q = lam * 2**-24`` is computed in float64, one numpy
operation per IEEE operation, and the candidate and tie rules are applied as the header states them."""
from __future__ import annotations

import numpy as np

from tests import rate_ref as R
from tests import synth as T

MAX_ABS = np.float32(2.0 ** 20)  # beyond it a latent keeps round(y)
SHAPES = [(8, 4, 4), (32, 16, 8), (12, 8, 13), (16, 16, 16)]  # tests/test_gpu_rate.py SHAPES
SEEDS = [(3, 0.0), (4, 0.5)]  # (seed, zero_frac) of tests/synth.make_latent
LAMBDAS = [0.0, 0.1, 0.5, 5.0]


def objective(y32, v32, cost_q, lam) -> np.ndarray:
    """J in float64: every operation a single IEEE binary64 operation"""
    lam_q = np.float64(lam) * np.float64(2.0 ** -24)
    d = y32.astype(np.float64) - v32.astype(np.float64)
    return d * d + lam_q * cost_q.astype(np.float64)


def rdoq(oracle, lib, mode, y, scales, means, weights, lam, clamp=True) -> dict:
    """y float32 [1, M, h, w], planes float32 [1, 4M, h, w] (weights: probabilities) -> what fgmm_gmc_rdoq_batch must return:
    ``y`` [1, M, h, w] float32, ``n_changed``, ``bits_q_before``, ``bits_q_after``, ``chan_after`` int64 [M], ``abs_max``,
    ``zero_bitmap`` (of ``y``), and for the tests' own conditions ``n_coded`` (latents of the coded channels), ``n_away`` (moves away
    from zero), ``n_bypass_cand`` (candidates priced as a bypass escape), ``j_before`` / ``j_after`` (float64 [n]: J of round(y) and of
    the choice)"""
    y = np.asarray(y, np.float32)
    _, M, h, w = y.shape
    hw = h * w
    sym0, s_, m_, w_, _, zb, _ = T.to_coder_inputs(y, scales, means, weights, clamp=clamp)
    nz = np.nonzero(zb)[0]
    out = {"chan_after": np.zeros(M, np.int64)}
    y_rdo = np.zeros_like(y)
    if len(sym0) == 0:
        out.update(y=y_rdo, n_changed=0, bits_q_before=0, bits_q_after=0, abs_max=1, zero_bitmap=zb.tolist(), n_coded=0, n_away=0,
                   n_bypass_cand=0, j_before=np.zeros(0), j_after=np.zeros(0), symbols=sym0)
        return out
    yv = y[0, nz].reshape(-1)
    with np.errstate(invalid="ignore"):
        v0 = np.round(yv)  # round half to even, float32
        cand = np.isfinite(yv) & (np.abs(v0) <= MAX_ABS)
    costs, vs, nbyp = [], [], 0
    for delta in (-1, 0, 1):
        sym = np.where(cand, sym0 + np.int32(delta), sym0).astype(np.int32) if delta else sym0
        packed = oracle.symtab(mode, sym, s_, m_, w_)
        _, _, c = R.host_bits(lib, packed, sym, costs=True)
        nbyp += int((((packed >> 16) == 0) & (cand | (delta == 0))).sum())
        costs.append(c)
        vs.append(v0 + np.float32(delta))
    with np.errstate(invalid="ignore"):
        jm, j0, jp = (objective(yv, v, c, lam) for v, c in zip(vs, costs))
        pick = np.zeros(len(sym0), np.int32)  # start from v0
        jb = j0.copy()
        take = cand & (jm < jb)  # v0 - 1 if strictly smaller
        pick[take], jb[take] = -1, jm[take]
        take = cand & (jp < jb)  # then v0 + 1 if strictly smaller than the best so far
        pick[take], jb[take] = 1, jp[take]
    chosen = (sym0 + pick).astype(np.int32)
    c_after = np.choose(pick + 1, costs)
    v_f = (v0 + pick.astype(np.float32)) + np.float32(0.0)  # (+0.0 for zero; NaN and +-inf latents stay what they are)
    y_rdo[0, nz] = v_f.reshape(len(nz), h, w)
    out["chan_after"][nz] = c_after.reshape(len(nz), hw).astype(np.int64).sum(1)
    sym_after, _, _, _, am, zb_after, _ = T.to_coder_inputs(y_rdo, scales, means, weights, clamp=clamp)
    out.update(y=y_rdo, n_changed=int((pick != 0).sum()), bits_q_before=int(costs[1].astype(np.uint64).sum()),
               bits_q_after=int(c_after.astype(np.uint64).sum()), abs_max=am, zero_bitmap=zb_after.tolist(), n_coded=len(sym0),
               n_away=int((np.abs(chosen.astype(np.int64)) > np.abs(sym0.astype(np.int64))).sum()), n_bypass_cand=nbyp, j_before=j0, j_after=jb,
               symbols=chosen)
    return out


def same_float_bits(a, b) -> bool:
    """equal as bit patterns, any NaN counting as equal to any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
