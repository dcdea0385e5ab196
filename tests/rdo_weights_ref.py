"""Shared by tests/test_rdo_weights_cpu.py and tests/test_gpu_rdo_weights.py: the reference side of the WEIGHTED distortion
(include/flashgmm_amd.h section 3e), numpy only, built on tests/rdoq_ref.py and tests/rdcurve_ref.py.

The candidates are priced as those modules price them (``rdcurve_ref.price``: the oracle's tables for ``sym - 1, sym, sym + 1``, entry
by entry through the library's HOST function ``fgmm_symtab_bits``).  The weight of the latent at channel ``c``, position ``p`` is
``float64(chan_w[c]) * float64(pos_w[p])`` - one multiply, exact; the objective ``J(v) = wt * (d * d) + lam_q * cost_q(v)`` and the
curve's ``rint((wt * inc) * 2**32)`` are computed in float64, one numpy operation per IEEE operation.  The candidate rule, the
strict-less order and the budget search (``rdcurve_ref.search``) are the unweighted ones."""
from __future__ import annotations

import numpy as np

from tests import rdcurve_ref as V
from tests import synth as T

LAM = 0.5  # the lambda of the non-vacuity conditions
CHAN_CYCLE = (0.25, 1.0, 4.0)
POS_CYCLE = (0.5, 1.0, 2.0, 1.0)


def chan_w(M) -> np.ndarray:
    """the tests' fixed channel factors: (0.25, 1, 4)[c % 3]"""
    return np.array([CHAN_CYCLE[c % 3] for c in range(M)], np.float32)


def pos_w(hw) -> np.ndarray:
    """the tests' fixed position factors: (0.5, 1, 2, 1)[p % 4]"""
    return np.array([POS_CYCLE[p % 4] for p in range(hw)], np.float32)


def weights_of(y, scales, means, weights, cw=None, pw=None, clamp=True) -> np.ndarray:
    """float64 [n]: the weight of every latent of the channels coded for y, in ``rdcurve_ref.price``'s order.  None: every factor 1"""
    y = np.asarray(y, np.float32)
    _, M, h, w = y.shape
    zb = T.to_coder_inputs(y, scales, means, weights, clamp=clamp)[5]
    nz = np.nonzero(zb)[0]
    cw = np.ones(M, np.float32) if cw is None else np.asarray(cw, np.float32).reshape(M)
    pw = np.ones(h * w, np.float32) if pw is None else np.asarray(pw, np.float32).reshape(h * w)
    return (cw[nz].astype(np.float64)[:, None] * pw.astype(np.float64)[None, :]).reshape(-1)  # ONE binary64 multiply per latent


def objective(y32, v32, cost_q, lam, wt) -> np.ndarray:
    """J in float64: three multiplies and one add, each a single IEEE binary64 operation"""
    lam_q = np.float64(lam) * np.float64(2.0 ** -24)
    d = y32.astype(np.float64) - v32.astype(np.float64)
    return wt * (d * d) + lam_q * cost_q.astype(np.float64)


def choose(priced, lam, wt):
    """-> (pick int32 [n] in -1 / 0 / +1, J of v0, J of the choice): the header's order v0, v0 - 1, v0 + 1, strictly less"""
    yv, vs, costs, cand = priced["yv"], priced["vs"], priced["costs"], priced["cand"]
    with np.errstate(invalid="ignore"):
        jm, j0, jp = (objective(yv, v, c, lam, wt) for v, c in zip(vs, costs))
        pick = np.zeros(len(yv), np.int32)
        jb = j0.copy()
        take = cand & (jm < jb)
        pick[take], jb[take] = -1, jm[take]
        take = cand & (jp < jb)
        pick[take], jb[take] = 1, jp[take]
    return pick, j0, jb


def rdoq(oracle, lib, mode, y, scales, means, weights, lam, clamp=True, cw=None, pw=None, priced=None) -> dict:
    """what fgmm_gmc_rdoq_batch_w must return, with ``rdoq_ref.rdoq``'s keys (less n_bypass_cand) and ``pick``; ``priced``: the
    latent's ``rdcurve_ref.price`` when the caller has it already"""
    y = np.asarray(y, np.float32)
    _, M, h, w = y.shape
    hw = h * w
    p = priced if priced is not None else V.price(oracle, lib, mode, y, scales, means, weights, clamp=clamp)
    sym0, _, _, _, _, zb, _ = T.to_coder_inputs(y, scales, means, weights, clamp=clamp)
    nz = np.nonzero(zb)[0]
    out = {"chan_after": np.zeros(M, np.int64)}
    y_rdo = np.zeros_like(y)
    if len(sym0) == 0:
        out.update(y=y_rdo, n_changed=0, bits_q_before=0, bits_q_after=0, abs_max=1, zero_bitmap=zb.tolist(), n_coded=0, n_away=0,
                   j_before=np.zeros(0), j_after=np.zeros(0), symbols=sym0, pick=np.zeros(0, np.int32))
        return out
    wt = weights_of(y, scales, means, weights, cw, pw, clamp=clamp)
    pick, j0, jb = choose(p, lam, wt)
    costs, v0 = p["costs"], p["vs"][1]
    chosen = (sym0 + pick).astype(np.int32)
    c_after = np.choose(pick + 1, costs)
    v_f = (v0 + pick.astype(np.float32)) + np.float32(0.0)  # (+0.0 for zero; NaN and +-inf latents stay what they are)
    y_rdo[0, nz] = v_f.reshape(len(nz), h, w)
    out["chan_after"][nz] = c_after.reshape(len(nz), hw).astype(np.int64).sum(1)
    _, _, _, _, am, zb_after, _ = T.to_coder_inputs(y_rdo, scales, means, weights, clamp=clamp)
    out.update(y=y_rdo, n_changed=int((pick != 0).sum()), bits_q_before=int(costs[1].astype(np.uint64).sum()),
               bits_q_after=int(c_after.astype(np.uint64).sum()), abs_max=am, zero_bitmap=zb_after.tolist(), n_coded=len(sym0),
               n_away=int((np.abs(chosen.astype(np.int64)) > np.abs(sym0.astype(np.int64))).sum()), j_before=j0, j_after=jb, symbols=chosen,
               pick=pick)
    return out


def curve(priced, lambdas, wt) -> dict:
    """what fgmm_gmc_rdcurve_batch_w must return: ``rdcurve_ref.curve``'s keys, ``ddist_q`` the weighted added distortion"""
    yv, vs, costs = priced["yv"], priced["vs"], priced["costs"]
    out = {"bits_q_before": int(costs[1].astype(np.uint64).sum()), "bits_q_after": [], "n_changed": [], "ddist_q": []}
    yd = yv.astype(np.float64)
    with np.errstate(invalid="ignore"):
        sq = [(yd - v.astype(np.float64)) * (yd - v.astype(np.float64)) for v in vs]  # dm * dm, d0 * d0, dp * dp
    for lam in lambdas:
        pick, _, _ = choose(priced, lam, wt)
        c_after = np.choose(pick + 1, costs) if len(yv) else np.zeros(0, np.uint32)
        moved = pick != 0
        inc = np.choose(pick + 1, sq)[moved] - sq[1][moved] if len(yv) else np.zeros(0)  # d * d - d0 * d0
        q = np.rint((wt[moved] * inc) * 2.0 ** 32) if len(yv) else np.zeros(0)  # round half to even
        assert np.all(q >= 0)
        out["bits_q_after"].append(int(c_after.astype(np.uint64).sum()))
        out["n_changed"].append(int(moved.sum()))
        out["ddist_q"].append(int(q.astype(np.uint64).sum()))
    return out


def group_f(lib, priced_items, wts):
    """f of a group under weights: lambdas -> [sum over the group's items of fgmm_rate_stream_bytes(bits_q_after at lambda)]"""
    def f(lambdas):
        cs = [curve(p, lambdas, wt)["bits_q_after"] for p, wt in zip(priced_items, wts)]
        return [sum(V.stream_bytes(lib, c[j]) for c in cs) for j in range(len(lambdas))]
    return f


def search(lib, priced_items, wts, budget, lambda_max=16.0, refine=2) -> dict:
    """the budget search of section 3d over the WEIGHTED decisions: ``rdcurve_ref.search`` itself, fed the weighted f"""
    return V.search(group_f(lib, priced_items, wts), budget, lambda_max=lambda_max, refine=refine)
