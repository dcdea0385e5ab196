"""GPU (-m gpu): the two bindings of the Python boundary - flashgmm_amd._native (csrc/fgmm_pybind.cpp) and its stand-in over ctypes
(flashgmm_amd/_boundary.py) - reached through the public methods of ``GaussianMixtureConditional``: every one of the nine callables
is called under either binding, and everything that comes back is the same - bytes, abs_max, bitmaps, y_q, notes, decoded latents, and
the integers and float bit patterns of the RDOQ, curve and budget results.  The shapes are the smallest at which the marshalling can
go wrong: item and bitmap-row strides that are not the dense ones, items of unlike shapes, more lambdas than one chunk, two groups."""
import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, ParameterHead, _boundary, _lib
from tests import synth as T
from tests.test_gpu_latent_calls import bkey, ckey, qkey

pytestmark = pytest.mark.gpu

NINE = {"compress_stacked", "compress_head_stacked", "decompress_stacked", "compress_items", "decompress_items", "rdoq_stacked", "rdoq_items",
        "rdcurve_items", "rdoq_budget_items"}
SEED = 5100  # (some stream of either form has two notes at stride 256: asserted)
N, M, H, W = 4, 8, 8, 12
SHAPES = [(8, 8, 12), (5, 3, 7), (16, 8, 8), (8, 8, 12), (5, 3, 7)]  # item 1 all-zero
LAMBDAS17 = [0.0] + [2.0 ** (k - 12) for k in range(16)]  # two chunks: 16 + 1


def dev(a):
    return torch.from_numpy(a).to("cuda:0")


def enc(res):
    """what a compress call returned, as values -> per item (type, bytes, abs_max, bitmap, y_q, notes, stride)"""
    return [(type(b), bytes(b), am, zb.tolist(), yq.cpu().numpy().tobytes()) + ((b.ckpt.tolist(), b.ckpt_stride) if isinstance(b, CheckpointedBytes) else ())
            for (b, am, zb), yq in res]


def skey(q):
    return qkey(q) + (q.n_skipped, q.n_eligible, None if q.skipped is None else q.skipped.tolist(), q.ddist_q)


def every_call(stride):
    """every public method that goes through the boundary -> {what: values}"""
    gmc = GaussianMixtureConditional(K=4, mode="polya", checkpoint_stride=stride)
    out = {}
    # ---- stacked ------------------------------------------------------------------------------------------------------------------------
    lat = [T.make_latent(SEED + i, M=M, h=H, w=W, clamp=False, zero_frac=0.2) for i in range(N)]
    ys, ss, ms, ws = (torch.cat([dev(l[k]) for l in lat]) for k in range(4))
    res = gmc.compress_batch(ys, ss, ms, ws)
    out["compress stacked"] = enc(res)
    assert torch.equal(res.y_q[:, 0], torch.round(ys)) and (not stride or max(len(b.ckpt) for b in res.strings) >= 2)
    for how, zbs in (("tensor", lambda s: res.zero_bitmaps[s::2]), ("list", lambda s: list(res.zero_bitmaps[s::2]))):
        stages = [gmc.decompress_batch(res.strings[s::2], res.abs_maxes[s::2], zbs(s), ss[s::2], ms[s::2], ws[s::2], stacked_output=True) for s in range(2)]
        assert all(torch.equal(stages[s], res.y_q[s::2]) for s in range(2)), how  # (two stage views: item stride 2 items, bitmap rows 2 M apart)
        out["decompress stacked, bitmaps as a " + how] = [t.cpu().numpy().tobytes() for t in stages]
    # ---- a sequence of unlike items -------------------------------------------------------------------------------------------------------
    mixed = [T.make_latent(SEED + 10 + i, M=m, h=h, w=w, clamp=False, zero_frac=1.0 if i == 1 else 0.2) for i, (m, h, w) in enumerate(SHAPES)]
    cols = [[dev(l[k]) for l in mixed] for k in range(4)]
    seq = gmc.compress_batch(*cols)
    out["compress items"] = enc(seq)
    assert seq[1][0][2].sum() == 0 and (not stride or max(len(r[0][0].ckpt) for r in seq) >= 2)
    back = gmc.decompress_batch([r[0][0] for r in seq], [r[0][1] for r in seq], [r[0][2] for r in seq], *cols[1:])
    assert all(torch.equal(b, r[1]) and torch.equal(b, torch.round(y)) for b, r, y in zip(back, seq, cols[0]))
    out["decompress items"] = [b.cpu().numpy().tobytes() for b in back]
    # ---- the fused head -------------------------------------------------------------------------------------------------------------------
    conv, x, yh = T.make_head(SEED + 20, M, 8, H, W, N)
    head = ParameterHead(conv)
    fused = gmc.compress_head_batch(yh, x, head)
    out["compress head"] = enc(fused)
    hb = gmc.decompress_batch(fused.strings, fused.abs_maxes, fused.zero_bitmaps, *head.params(x), weights_are_logits=True, stacked_output=True)
    assert torch.equal(hb, fused.y_q) and torch.equal(hb[:, 0], torch.round(yh))
    # ---- the calls that price latents -------------------------------------------------------------------------------------------------------
    out["rdoq stacked"] = [qkey(q) for q in gmc.quantize_rdo_batch(ys, ss, ms, ws, 0.5)]
    out["rdoq stacked, per channel"] = [qkey(q) for q in gmc.quantize_rdo_batch(ys, ss, ms, ws, 0.5, per_channel=True)]
    cw = [torch.linspace(0.5, 2.0, m, device="cuda:0") for m, _, _ in SHAPES]
    pw = [torch.linspace(0.25, 4.0, h * w, device="cuda:0").reshape(h, w) for _, h, w in SHAPES]
    out["rdoq items, weighted, channel skip"] = [skey(q) for q in gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True, channel_weights=cw,
                                                                                          position_weights=pw, channel_skip=True)]
    curves = gmc.rd_curve_batch(ys, ss, ms, ws, LAMBDAS17)
    out["rd curve, 17 lambdas"] = [ckey(c) for c in curves]
    assert all(len(c.bits_q_after) == 17 and c.bits_q_after[0] == c.bits_q_before for c in curves)
    groups = [0, 1, 1, 0]
    budgets = [(sum(curves[i].nbytes[0] for i in mem) + sum(curves[i].nbytes[-1] for i in mem)) // 2 for mem in ((0, 3), (1, 2))]
    out["budget, two groups"] = [bkey(q) for q in gmc.quantize_to_budget_batch(ys, ss, ms, ws, budgets, groups=groups, per_channel=True)]
    # ---- nothing to do ----------------------------------------------------------------------------------------------------------------------
    none = gmc.compress_batch(ys[:0], ss[:0], ms[:0], ws[:0])
    assert len(none) == 0 and none.strings == [] and none.abs_maxes == [] and none.zero_bitmaps.shape == (0, M) and none.y_q.shape == (0, 1, M, H, W)
    assert gmc.decompress_batch([], [], none.zero_bitmaps, ss[:0], ms[:0], ws[:0]) == [] and gmc.decompress_batch([], [], [], ss[:0], ms[:0], ws[:0]) == []
    assert gmc.decompress_batch([], [], [], ss[:0], ms[:0], ws[:0], stacked_output=True).shape == (0, 1, M, H, W)
    assert gmc.compress_batch([], [], [], []) == [] and gmc.decompress_batch([], [], [], [], [], []) == []
    assert len(gmc.compress_head_batch(yh[:0], x[:0], head)) == 0 and gmc.quantize_rdo_batch(ys[:0], ss[:0], ms[:0], ws[:0], 0.5) == []
    return out


@pytest.mark.parametrize("stride", [0, 256])
def test_every_boundary_call_gives_the_same_under_both_bindings(monkeypatch, stride):
    nat = _lib.native()
    assert nat is not None, "flashgmm_amd/_native*.so is missing: flashgmm_amd/csrc/build.sh builds it"
    reached = set()

    def counted(name, fn):
        def call(*a, **k):
            reached.add(name)
            return fn(*a, **k)
        return call

    class Counted:  # the compiled module with every callable counted (substituted through _lib.native)
        pass

    proxy = Counted()
    for name in NINE:
        setattr(proxy, name, counted(name, getattr(nat, name)))
        monkeypatch.setattr(_boundary, name, counted(name, getattr(_boundary, name)))
    monkeypatch.setattr(_lib, "native", lambda: proxy)
    compiled = every_call(stride)
    assert reached == NINE and _lib.boundary() is proxy
    reached.clear()
    monkeypatch.setattr(_lib, "native", lambda: None)
    assert _lib.boundary() is _boundary
    ctypes_ = every_call(stride)
    assert reached == NINE
    assert list(compiled) == list(ctypes_)
    for what in compiled:
        assert compiled[what] == ctypes_[what], what
    assert all(t is (CheckpointedBytes if stride else bytes) for t, *_ in compiled["compress stacked"] + compiled["compress items"] + compiled["compress head"])
    assert any(k[1] > 0 for k in compiled["rdoq stacked"]) and any(k[-4] > 0 for k in compiled["budget, two groups"])
