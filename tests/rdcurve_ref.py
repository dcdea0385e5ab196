"""Shared by tests/test_rdcurve_cpu.py and tests/test_gpu_rdcurve.py: the reference side of the rate-distortion curve and of the
budget search (include/flashgmm_amd.h section 3d), numpy only, built on tests/rdoq_ref.py.

The three candidates of every latent of a coded channel are priced ONCE, as tests/rdoq_ref.py prices them (the oracle's tables for
``sym - 1, sym, sym + 1``, entry by entry through the library's HOST function ``fgmm_symtab_bits``); per lambda the objective
(``rdoq_ref.objective``) and the header's choice are applied.  ``ddist_q`` is computed in float64 one IEEE operation at a time.  The
budget search is restated as the header words it, with ``f`` supplied by the curve."""
from __future__ import annotations

import ctypes as C

import numpy as np

from tests import rate_ref as R
from tests import rdoq_ref as Q
from tests import synth as T

# the budget tests' cases: rdoq_ref.SHAPES x SEEDS with ONE seed replaced.  At (8, 4, 4), seed 3, polya, the budget's threshold lies in the
# last sixteenth below a point of the round-0 grid (lambda* = 0.0625 = 16 * 2^-8 exactly), so no refinement round moves hi and the case
# would not show that refinement works; seed 5 at that shape moves hi in both rounds in every mode (tests/test_rdcurve_cpu.py asserts it)
BUDGET_CASES = [(shape, (5, 0.0) if (shape, sz) == ((8, 4, 4), (3, 0.0)) else sz) for shape in Q.SHAPES for sz in Q.SEEDS]
N_MAX = 16  # FGMM_RDCURVE_MAX
BUDGET_UNMET = 7  # FGMM_BUDGET_UNMET


def budget_cases(clamp):
    """-> [(y, scales, means, weights)] of BUDGET_CASES"""
    return [T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf) for shape, (seed, zf) in BUDGET_CASES]


def budget_of(b0, b16) -> int:
    """the tests' budget between bytes(lambda = 0) and bytes(lambda = 16): half way, rounded down to a multiple of 4"""
    return ((b0 + b16) // 2) // 4 * 4


def price(oracle, lib, mode, y, scales, means, weights, clamp=True) -> dict:
    """y float32 [1, M, h, w], planes float32 [1, 4M, h, w] (weights: probabilities) -> the latents of the coded channels priced:
    ``yv`` float32 [n], ``vs`` / ``costs``: round(y) - 1, round(y), round(y) + 1 and their cost_q (the neighbours of a latent that is
    not a candidate are never chosen), ``cand`` bool [n]"""
    y = np.asarray(y, np.float32)
    sym0, s_, m_, w_, _, zb, _ = T.to_coder_inputs(y, scales, means, weights, clamp=clamp)
    nz = np.nonzero(zb)[0]
    if len(sym0) == 0:
        z = np.zeros(0, np.float32)
        return {"yv": z, "vs": [z, z, z], "costs": [np.zeros(0, np.uint32)] * 3, "cand": np.zeros(0, bool)}
    yv = y[0, nz].reshape(-1)
    with np.errstate(invalid="ignore"):
        v0 = np.round(yv)  # round half to even, float32
        cand = np.isfinite(yv) & (np.abs(v0) <= Q.MAX_ABS)
    costs, vs = [], []
    for delta in (-1, 0, 1):
        sym = np.where(cand, sym0 + np.int32(delta), sym0).astype(np.int32) if delta else sym0
        packed = oracle.symtab(mode, sym, s_, m_, w_)
        _, _, c = R.host_bits(lib, packed, sym, costs=True)
        costs.append(c)
        vs.append(v0 + np.float32(delta))
    return {"yv": yv, "vs": vs, "costs": costs, "cand": cand}


def curve(priced, lambdas) -> dict:
    """-> what fgmm_gmc_rdcurve_batch must return: ``bits_q_before``, and per lambda ``bits_q_after``, ``n_changed``, ``ddist_q`` (lists of ints)"""
    yv, vs, costs, cand = priced["yv"], priced["vs"], priced["costs"], priced["cand"]
    out = {"bits_q_before": int(costs[1].astype(np.uint64).sum()), "bits_q_after": [], "n_changed": [], "ddist_q": []}
    yd = yv.astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = [yd - v.astype(np.float64) for v in vs]  # dm, d0, dp
        sq = [x * x for x in d]
    for lam in lambdas:
        with np.errstate(invalid="ignore"):
            jm, j0, jp = (Q.objective(yv, v, c, lam) for v, c in zip(vs, costs))
            pick = np.zeros(len(yv), np.int32)  # start from v0
            jb = j0.copy()
            take = cand & (jm < jb)  # v0 - 1 if strictly smaller
            pick[take], jb[take] = -1, jm[take]
            take = cand & (jp < jb)  # then v0 + 1 if strictly smaller than the best so far
            pick[take] = 1
        c_after = np.choose(pick + 1, costs) if len(yv) else np.zeros(0, np.uint32)
        moved = pick != 0
        inc = np.choose(pick + 1, sq)[moved] - sq[1][moved] if len(yv) else np.zeros(0)  # d * d - d0 * d0
        q = np.rint(inc * 2.0 ** 32)  # round half to even
        assert np.all(q >= 0)
        out["bits_q_after"].append(int(c_after.astype(np.uint64).sum()))
        out["n_changed"].append(int(moved.sum()))
        out["ddist_q"].append(int(q.astype(np.uint64).sum()))
    return out


def stream_bytes(lib, bits_q) -> int:
    return int(lib.fgmm_rate_stream_bytes(C.c_uint64(int(bits_q))))


def group_f(lib, priced_items):
    """f of a group: lambdas -> [sum over the group's items of fgmm_rate_stream_bytes(bits_q_after at lambda)]"""
    def f(lambdas):
        cs = [curve(p, lambdas)["bits_q_after"] for p in priced_items]
        return [sum(stream_bytes(lib, c[j]) for c in cs) for j in range(len(lambdas))]
    return f


def search(f, budget, lambda_max=16.0, refine=2) -> dict:
    """the budget search of header section 3d; ``f(list of lambdas) -> list of bytes``.  -> ``lam``, ``bytes_pred``, ``passes``,
    ``status`` (0 or BUDGET_UNMET), and for the tests' own conditions ``f_before`` (f at the point before ``lam`` in the final grid, None
    when there is none) and ``moved`` (refinement rounds that moved hi)"""
    lambda_max = np.float64(lambda_max)
    grid = [np.float64(0.0)] + [lambda_max * np.float64(2.0 ** (j - 15)) for j in range(1, N_MAX)]
    fg = f(grid)
    passes, moved = 1, 0
    feas = [j for j in range(N_MAX) if fg[j] <= budget]
    if not feas:
        return {"lam": float(lambda_max), "bytes_pred": fg[N_MAX - 1], "passes": passes, "status": BUDGET_UNMET, "f_before": None, "moved": 0}
    j = feas[0]
    if j == 0:
        return {"lam": 0.0, "bytes_pred": fg[0], "passes": passes, "status": 0, "f_before": None, "moved": 0}
    lo, hi, f_hi, f_lo = grid[j - 1], grid[j], fg[j], fg[j - 1]
    for _ in range(refine):
        if lo == hi:
            break
        grid = [lo + (hi - lo) * np.float64(k) / np.float64(16.0) for k in range(1, N_MAX)] + [hi]
        fg = f(grid)
        passes += 1
        if fg[N_MAX - 1] > budget:  # hi, evaluated again, no longer fits: lo and hi stay, the search stops
            break
        k = [i for i in range(N_MAX) if fg[i] <= budget][0]
        if k > 0:
            lo, f_lo = grid[k - 1], fg[k - 1]
        moved += grid[k] != hi
        hi, f_hi = grid[k], fg[k]
    return {"lam": float(hi), "bytes_pred": f_hi, "passes": passes, "status": 0, "f_before": f_lo, "moved": moved}
