"""Shared by tests/test_rdo_skip_cpu.py and tests/test_gpu_rdo_skip.py: the reference side of CHANNEL SKIPPING (include/flashgmm_amd.h
section 3f), numpy only, built on tests/rdo_weights_ref.py and tests/rdcurve_ref.py.

The per-latent decisions are those modules' (``rdo_weights_ref.choose`` over ``rdcurve_ref.price``).  Per channel the header's sums are
taken as integers - ``A``, ``nzA``, ``nz0``, ``Dk`` (units of 2^-32) and ``Dz`` (units of 2^-16, ``incz = dz * dz - d0 * d0``) - and the
rule ``skip = !inelig && (nzA == 0 || Jz < Jk)`` with ``Jk = float64(Dk) * 2^-32 + lam_q * float64(A)`` and ``Jz = float64(Dz) * 2^-16``
is evaluated in float64, one numpy operation per IEEE operation.  The budget search is ``rdcurve_ref.search`` itself, fed the skip-form f."""
from __future__ import annotations

import numpy as np

from tests import rdcurve_ref as V
from tests import rdo_weights_ref as W
from tests import synth as T

VMAX = 15  # FGMM_SKIP_VMAX
HW_MAX = 1 << 24
MASK64 = (1 << 64) - 1


def channels(priced, lam, wt, hw) -> dict:
    """the sums and the decision of every coded channel at ``lam`` -> arrays over the coded channels, in ``rdcurve_ref.price``'s order:
    ``A``, ``nzA``, ``nz0``, ``Dk``, ``Dz`` (uint64), ``moved`` (latents moved, int64), ``inelig``, ``vmax`` (ineligible through
    ``|v0| > 15``), ``skip`` (bool), and ``pick`` (int32 [n], the per-latent choice)"""
    yv, vs, costs = priced["yv"], priced["vs"], priced["costs"]
    n = len(yv)
    nch = n // hw if hw else 0
    pick, _, _ = W.choose(priced, lam, wt)
    v0 = vs[1]
    yd = yv.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sq = [(yd - v.astype(np.float64)) * (yd - v.astype(np.float64)) for v in vs]  # dm * dm, d0 * d0, dp * dp
        moved = pick != 0
        inc = np.choose(pick + 1, sq) - sq[1]  # d * d - d0 * d0
        qk = np.where(moved, np.rint((wt * np.where(moved, inc, 0.0)) * 2.0 ** 32), 0.0)
        finite = np.isfinite(yv)
        over = finite & (np.abs(v0) > np.float32(VMAX))
        big = ~finite | over
        nz = v0 != 0  # (NaN != 0: its channel is ineligible anyway)
        term = nz & ~big
        incz = yd * yd - sq[1]  # dz * dz - d0 * d0, dz = float64(y)
        qz = np.where(term, np.rint((wt * np.where(term, incz, 0.0)) * 2.0 ** 16), 0.0)
        chosen = v0 + pick.astype(np.float32)
    assert np.all(qk >= 0) and np.all(qz >= 0)

    def per(a, dtype=np.uint64):
        return a.astype(dtype).reshape(nch, hw).sum(1, dtype=dtype)

    A, Dk, Dz = per(np.choose(pick + 1, costs)), per(qk), per(qz)
    nzA, nz0 = per(chosen != 0), per(nz)
    inelig = big.reshape(nch, hw).any(1) | (hw > HW_MAX)
    lam_q = np.float64(lam) * np.float64(2.0 ** -24)
    jk = Dk.astype(np.float64) * np.float64(2.0 ** -32) + lam_q * A.astype(np.float64)
    jz = Dz.astype(np.float64) * np.float64(2.0 ** -16)
    skip = ~inelig & ((nzA == 0) | (jz < jk))
    return {"A": A, "nzA": nzA, "nz0": nz0, "Dk": Dk, "Dz": Dz, "moved": per(moved, np.int64), "inelig": inelig,
            "vmax": over.reshape(nch, hw).any(1), "skip": skip, "pick": pick}


def sums(ch) -> dict:
    """the item's sums after the channel decisions of ``channels``"""
    k, z = ~ch["skip"], ch["skip"]
    dd = sum(int(v) for v in ch["Dk"][k]) + sum(int(v) << 16 for v in ch["Dz"][z])
    return {"bits_q_after": int(ch["A"][k].sum(dtype=np.uint64)), "n_changed": int(ch["moved"][k].sum()) + int(ch["nz0"][z].sum()),
            "ddist_q": dd & MASK64, "n_skipped": int(z.sum()), "n_eligible": int((~ch["inelig"]).sum())}


def rdoq(oracle, lib, mode, y, scales, means, weights, lam, clamp=True, cw=None, pw=None, priced=None) -> dict:
    """what fgmm_gmc_rdoq_batch_s must return with a skip array: ``rdo_weights_ref.rdoq``'s keys ``y``, ``n_changed``, ``bits_q_before``,
    ``bits_q_after``, ``chan_after``, ``abs_max``, ``zero_bitmap``, and ``n_skipped``, ``n_eligible``, ``ddist_q``, ``skipped`` (bool [M]);
    for the tests' own conditions ``ch`` (``channels``) and ``coded`` (the coded channels' indices)"""
    y = np.asarray(y, np.float32)
    _, M, h, w = y.shape
    hw = h * w
    p = priced if priced is not None else V.price(oracle, lib, mode, y, scales, means, weights, clamp=clamp)
    base = W.rdoq(oracle, lib, mode, y, scales, means, weights, lam, clamp=clamp, cw=cw, pw=pw, priced=p)
    zb = T.to_coder_inputs(y, scales, means, weights, clamp=clamp)[5]
    nz = np.nonzero(zb)[0]
    out = {"bits_q_before": base["bits_q_before"], "skipped": np.zeros(M, bool), "coded": nz}
    if len(p["yv"]) == 0:
        out.update(y=base["y"], n_changed=0, bits_q_after=0, chan_after=base["chan_after"], abs_max=base["abs_max"], zero_bitmap=base["zero_bitmap"],
                   n_skipped=0, n_eligible=0, ddist_q=0, ch=None)
        return out
    ch = channels(p, lam, W.weights_of(y, scales, means, weights, cw, pw, clamp=clamp), hw)
    assert np.array_equal(ch["pick"], base["pick"]) and np.array_equal(ch["A"].astype(np.int64), base["chan_after"][nz])
    y_rdo, chan_after = base["y"].copy(), base["chan_after"].copy()
    y_rdo[0, nz[ch["skip"]]] = np.float32(0.0)  # +0.0
    chan_after[nz[ch["skip"]]] = 0
    out["skipped"][nz[ch["skip"]]] = True
    _, _, _, _, am, zb_after, _ = T.to_coder_inputs(y_rdo, scales, means, weights, clamp=clamp)
    out.update(sums(ch), y=y_rdo, chan_after=chan_after, abs_max=am, zero_bitmap=zb_after.tolist(), ch=ch)
    return out


def curve(priced, lambdas, wt, hw) -> dict:
    """what fgmm_gmc_rdcurve_batch_s must return with a skip array: ``rdcurve_ref.curve``'s keys after the channel decisions, and
    ``n_skipped`` per lambda, ``n_eligible``"""
    out = {"bits_q_before": int(priced["costs"][1].astype(np.uint64).sum()), "bits_q_after": [], "n_changed": [], "ddist_q": [], "n_skipped": [],
           "n_eligible": 0}
    for lam in lambdas:
        if len(priced["yv"]) == 0:
            s = {"bits_q_after": 0, "n_changed": 0, "ddist_q": 0, "n_skipped": 0, "n_eligible": 0}
        else:
            s = sums(channels(priced, lam, wt, hw))
        for k in ("bits_q_after", "n_changed", "ddist_q", "n_skipped"):
            out[k].append(s[k])
        out["n_eligible"] = s["n_eligible"]
    return out


def group_f(lib, priced_items, wts, hws):
    """the skip-form f of a group: lambdas -> [sum over the group's items of fgmm_rate_stream_bytes(bits_q_after at lambda)]"""
    def f(lambdas):
        cs = [curve(p, lambdas, wt, hw)["bits_q_after"] for p, wt, hw in zip(priced_items, wts, hws)]
        return [sum(V.stream_bytes(lib, c[j]) for c in cs) for j in range(len(lambdas))]
    return f


def search(lib, priced_items, wts, hws, budget, lambda_max=16.0, refine=2) -> dict:
    """the budget search of section 3d over the decisions of section 3f: ``rdcurve_ref.search`` itself, fed the skip-form f"""
    return V.search(group_f(lib, priced_items, wts, hws), budget, lambda_max=lambda_max, refine=refine)
