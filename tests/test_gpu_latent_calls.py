"""GPU (-m gpu): the four calls that price latents - ``estimate_bits_batch``, ``quantize_rdo_batch``, ``rd_curve_batch`` and
``quantize_to_budget_batch`` - over a BATCH of unlike items, held to the same calls on each item alone.  What a single item gives is
pinned to the oracle by test_gpu_rate.py, test_gpu_rdoq.py, test_gpu_rdcurve.py and test_gpu_enc_frame.py; what those leave open is
the calls' common front half on the host (flashgmm_amd/csrc/fgmm_estimate.cpp, LatentFrame) once the items differ: the batch's maxima,
every item's workspace offsets, the batch-wide choice of load width and grid, the descriptor offset of the per-lambda launches, the
workspace the budget call's RDOQ run takes over from the curve passes - and the Python item builder's two input forms.  Everything
is an integer or a float's bit pattern: every comparison is for EQUALITY.

  batch A  (16, 16, 16), (4, 16, 32)                    every hw a multiple of 256: the linear grid, 4-wide; fp32 and fp16 planes
  batch B  (8, 4, 4), M = 0, (12, 8, 13), (16, 16, 16)  the tiled grid, 4-wide; an empty item in the middle; unequal M and hw
  batch C  batch B, the (12, 8, 13) item's y one float into its storage: the whole batch 1-wide, tiled (hw = 16)"""
import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from tests import enc_ref as F
from tests import rdcurve_ref as V
from tests import synth as T
from tests.test_gpu_enc_frame import dv

pytestmark = pytest.mark.gpu

SEED = 40  # item i of a batch is drawn from SEED + i: 0 < coded channels < M at every shape below (asserted)
LAMBDAS = [0.0, 0.1, 0.5, 16.0]
A = [(16, 16, 16), (4, 16, 32)]
B = [(8, 4, 4), (0, 4, 4), (12, 8, 13), (16, 16, 16)]
BATCHES = {"A": (A, False, None), "A fp16": (A, True, None), "B": (B, False, None), "C": (B, False, 2)}
FORMS = {"A": (4, F.LIN), "A fp16": (4, F.LIN), "B": (4, F.TILED), "C": (1, F.TILED)}  # asserted on the batch's tensors


def make_batch(shapes, f16=False, off=None):
    """-> four lists (y, scales, means, weights) of device tensors; item ``off``'s y sits one float into its storage"""
    cols = [[], [], [], []]
    for i, (M, h, w) in enumerate(shapes):
        y, s, m, pi = T.make_latent(SEED + i, M, h, w, clamp=False, zero_frac=0.5)
        assert M == 0 or 0 < int((np.abs(np.round(y)).sum((3, 2))[0] != 0).sum()) < M, (M, h, w)
        planes = T.to_float16_planes(s, m, pi) if f16 else (s, m, pi)
        for col, a in zip(cols, (y, *planes)):
            col.append(dv(a, off == i and a is y))
    return cols


def bits(t):
    return None if t is None else t.cpu().numpy().tobytes()


def ekey(e):
    return (e.bits_q, e.nbytes, e.n_symbols, e.n_bypass, e.abs_max, bits(e.zero_bitmap), bits(e.channel_bits_q), bits(e.latent_bits))


def qkey(q):
    return (bits(q.y), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, bits(q.zero_bitmap), bits(q.channel_bits_q_after))


def ckey(c):
    return (c.lambdas, c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q, c.n_symbols)


def bkey(q):
    return qkey(q) + (q.lam, q.bytes_pred, q.passes, q.budget_met)


def item(cols, i):
    return [col[i] for col in cols]


@pytest.mark.parametrize("name", list(BATCHES))
def test_a_batch_is_its_items(name):
    shapes, f16, off = BATCHES[name]
    gmc = GaussianMixtureConditional(K=4, mode="polya", clamp_scales=True)
    cols = make_batch(shapes, f16, off)
    n = len(shapes)
    assert F.form_of(*cols) == FORMS[name]
    # ---- the batch against single items ------------------------------------------------------------------------------------------------
    est = gmc.estimate_bits_batch(*cols, per_channel=True, per_latent=True)
    assert [ekey(e) for e in est] == [ekey(gmc.estimate_bits(*item(cols, i), per_channel=True, per_latent=True)) for i in range(n)]
    rdo = gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True)
    assert [qkey(q) for q in rdo] == [qkey(gmc.quantize_rdo(*item(cols, i), 0.5, per_channel=True)) for i in range(n)]
    assert any(q.n_changed > 0 for q in rdo)
    curves = gmc.rd_curve_batch(*cols, LAMBDAS)
    assert [ckey(c) for c in curves] == [ckey(gmc.rd_curve(*item(cols, i), LAMBDAS)) for i in range(n)]
    assert [c.nbytes[0] for c in curves] == [e.nbytes for e in est]  # (the empty item: 8)
    # ---- to a budget, every item its own group: half way between its bytes at lambda = 0 and at 16 ----------------------------------
    budgets = [V.budget_of(c.nbytes[0], c.nbytes[-1]) if M else 8 for c, (M, _, _) in zip(curves, shapes)]
    own = gmc.quantize_to_budget_batch(*cols, budgets, per_channel=True)
    assert [bkey(q) for q in own] == [bkey(gmc.quantize_to_budget(*item(cols, i), budgets[i], per_channel=True)) for i in range(n)]
    assert any(q.lam > 0 for q in own)
    # ---- grouped: one lambda and one budget per group, on the sum of its items' bytes -------------------------------------------------
    groups = [i // 2 for i in range(n)]
    members = [[i for i in range(n) if groups[i] == g] for g in range(groups[-1] + 1)]
    budgets = [V.budget_of(sum(curves[i].nbytes[0] for i in mem), sum(curves[i].nbytes[-1] for i in mem)) for mem in members]
    got = gmc.quantize_to_budget_batch(*cols, budgets, groups=groups, per_channel=True)
    stream_bytes = _lib.lib().fgmm_rate_stream_bytes
    for g, mem in enumerate(members):
        lam = got[mem[0]].lam
        at_lam = gmc.quantize_rdo_batch(*cols, lam, per_channel=True)
        for i in mem:
            assert (got[i].lam, qkey(got[i])) == (lam, qkey(at_lam[i])), (g, i)
            assert got[i].bytes_pred == sum(int(stream_bytes(got[k].bits_q_after)) for k in mem), (g, i)
    assert any(q.lam > 0 for q in got)


def test_the_sequence_form_and_the_stacked_form_agree(monkeypatch):
    """two (16, 16, 16) items as lists and as stacked [2, ...] tensors, through the compiled boundary as built and through ctypes"""
    gmc = GaussianMixtureConditional(K=4, mode="polya", clamp_scales=True)
    cols = make_batch([A[0], A[0]])
    stacked = [torch.cat(col) for col in cols]
    at0, at16 = (sum(v) for v in zip(*(c.nbytes[::3] for c in gmc.rd_curve_batch(*cols, LAMBDAS))))
    assert at0 > at16
    budget = V.budget_of(at0, at16)  # (takes a search: lambda > 0)
    want = None
    for native in (True, False):
        if not native:
            monkeypatch.setattr(_lib, "native", lambda: None)
        for form in (cols, stacked):
            got = ([ekey(e) for e in gmc.estimate_bits_batch(*form, per_channel=True, per_latent=True)],
                   [qkey(q) for q in gmc.quantize_rdo_batch(*form, 0.5, per_channel=True)],
                   [ckey(c) for c in gmc.rd_curve_batch(*form, LAMBDAS)],
                   [bkey(q) for q in gmc.quantize_to_budget_batch(*form, budget, groups=[0, 0], per_channel=True)])
            want = want or got
            assert got == want, (native, form is stacked)
