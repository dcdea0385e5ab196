"""GPU (-m gpu): channel skipping for RDOQ, the curve and the budget search (include/flashgmm_amd.h section 3f; the SKIP instantiations
of rdoq_kernel and rdcurve_kernel, rdoq_skip_kernel, the skip form of rdcurve_fold_kernel) against tests/rdo_skip_ref.py.  Every output
is compared for EQUALITY: the chosen latents bit for bit, the counts, the integer sums, the flags.  That the sweep's cases skip a
channel, keep an eligible one and meet a channel beyond FGMM_SKIP_VMAX is checked on the CPU by tests/test_rdo_skip_cpu.py.  Shapes:
tests/rdoq_ref.SHAPES (hw = 16 less than a wave, hw = 104 a partial wave, both 4-wide on the tiled grid, hw = 256 a whole block on the
linear grid), and BIG, the smallest 4-wide plane that spans two workgroups; 1-wide only where a tensor is handed over misaligned.  Planes
with hw % 4 != 0: tests/test_gpu_enc_forms.py.  Where a comment names a launch form, ``enc_ref.form_of`` asserts it on the call's tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import BudgetQuantized, GaussianMixtureConditional, RdCurve, RdoQuantized, _lib
from tests import enc_ref as F
from tests import rdcurve_ref as V
from tests import rdo_skip_ref as S
from tests import rdo_weights_ref as W
from tests import rdoq_ref as Q
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
LAMBDAS16 = [0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 16.0]
K_BLOCK = 256  # kBlock (flashgmm_amd/csrc/fgmm_dev.h): a workgroup takes kBlock * VEC positions of a channel
BIG = (4, 4, (K_BLOCK * 4 + 4) // 4)  # M = 4, hw = 1028: the smallest multiple of VEC = 4 above one workgroup's 1024 positions


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def misaligned(a):
    """the same values in a view that starts one element into its storage: not 16-byte aligned, so the batch goes 1-wide"""
    buf = torch.zeros(a.numel() + 1, dtype=a.dtype, device=a.device)
    buf[1:] = a.reshape(-1)
    v = buf[1:].view(a.shape)
    assert v.data_ptr() % 16 == 4
    return v


def check(got, ref, name):
    assert isinstance(got, RdoQuantized)
    y = got.y.cpu().numpy()
    assert Q.same_float_bits(y, ref["y"]), (name, int((y.view(np.uint32) != ref["y"].view(np.uint32)).sum()))
    assert (got.n_changed, got.bits_q_before, got.bits_q_after) == (ref["n_changed"], ref["bits_q_before"], ref["bits_q_after"]), name
    assert (got.abs_max, got.zero_bitmap.tolist()) == (ref["abs_max"], ref["zero_bitmap"]), name
    assert (got.n_skipped, got.n_eligible, got.ddist_q) == (ref["n_skipped"], ref["n_eligible"], ref["ddist_q"]), name
    if got.channel_bits_q_after is not None:
        assert got.channel_bits_q_after.tolist() == ref["chan_after"].tolist(), name
        assert got.skipped.dtype == torch.bool and got.skipped.tolist() == ref["skipped"].tolist(), name


def key(q):
    return (q.y.cpu().numpy().tobytes(), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, q.zero_bitmap.tolist(),
            None if q.channel_bits_q_after is None else q.channel_bits_q_after.tolist())


def skey(q):
    return key(q) + (q.n_skipped, q.n_eligible, q.ddist_q, None if q.skipped is None else q.skipped.tolist())


def bkey(q):
    return key(q) + (q.lam, q.bytes_pred, q.budget_met, q.passes)


def ckey(c):
    return (c.lambdas, c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q, c.n_symbols)


def make_cases(clamp):
    return [T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf) for shape in Q.SHAPES for seed, zf in Q.SEEDS]


_PRICED = {}


def priced_cases(oracle, mode, clamp):
    """the sweep's eight cases and BIG, their fixed weights and their candidates priced - once per (mode, clamp), shared by the tests"""
    k = (mode, clamp)
    if k not in _PRICED:
        cases = make_cases(clamp) + [T.make_latent(7, *BIG, clamp=not clamp)]
        cws = [W.chan_w(c[0].shape[1]) for c in cases]
        pws = [W.pos_w(c[0].shape[2] * c[0].shape[3]).reshape(c[0].shape[2:]) for c in cases]
        priced = [V.price(oracle, _lib.lib(), mode, *c, clamp=clamp) for c in cases]
        wts = [W.weights_of(*c, cw, pw, clamp=clamp) for c, cw, pw in zip(cases, cws, pws)]
        ones = [W.weights_of(*c, clamp=clamp) for c in cases]
        hws = [c[0].shape[2] * c[0].shape[3] for c in cases]
        _PRICED[k] = (cases, cws, pws, priced, wts, ones, hws)
    return _PRICED[k]


# ---- 1. quantize_rdo with channel skipping ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_skip_quantize_rdo_against_the_reference(oracle, mode, clamp, weighted):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases, cws, pws, priced, _, _, hws = priced_cases(oracle, mode, clamp)
    n8 = len(cases) - 1  # the mixed batch: the eight cases; BIG goes alone, on its own grid
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    cw_d, pw_d = [dv(a) for a in cws], [dv(a) for a in pws]

    def kw(sel, pos=None):
        if not weighted:
            return dict(channel_skip=True, per_channel=True)
        return dict(channel_skip=True, per_channel=True, channel_weights=[cw_d[i] for i in sel], position_weights=[pw_d[i] for i in sel] if pos is None else pos)

    any_skipped = False
    for lam in Q.LAMBDAS:
        refs = [S.rdoq(oracle, L, mode, *c, lam, clamp=clamp, cw=cw if weighted else None, pw=pw if weighted else None, priced=p)
                for c, cw, pw, p in zip(cases, cws, pws, priced)]
        pos = (lambda sel: [pw_d[i] for i in sel]) if weighted else (lambda sel: None)
        assert F.form_of(*(col[:n8] for col in cols), pos_w=pos(range(n8))) == F.form_of(*(col[n8:] for col in cols), pos_w=pos([n8])) == (4, F.TILED)
        got = gmc.quantize_rdo_batch(*(col[:n8] for col in cols), lam, **kw(range(n8)))  # mixed shapes
        got += gmc.quantize_rdo_batch(*(col[n8:] for col in cols), lam, **kw([n8]))  # two workgroups per channel
        assert len(got) == len(cases)
        for i, (g, r) in enumerate(zip(got, refs)):
            check(g, r, (lam, i))
            if lam == 0.0:
                assert g.n_changed == 0 and g.n_skipped == 0 and g.bits_q_after == g.bits_q_before
            any_skipped = any_skipped or g.n_skipped > 0
        # single calls (each shape on its own grid)
        singles = [gmc.quantize_rdo(*(col[i] for col in cols), lam, channel_skip=True, per_channel=True, channel_weights=cw_d[i] if weighted else None,
                                    position_weights=pw_d[i] if weighted else None) for i in range(n8)]
        assert [skey(s) for s in singles] == [skey(g) for g in got[:n8]], lam
        # the 1-wide path: a pos_w that is not 16-byte aligned (weighted), a latent that is not (unweighted) - BIG included
        for i in (3, 4, 6, n8):
            linear = hws[i] % 64 == 0  # (1-wide: a wave takes 64 positions)
            if weighted:
                off = misaligned(pw_d[i])
                assert F.form_of_one(*(col[i] for col in cols), pos_w=off) == (1, linear)
                s = gmc.quantize_rdo(*(col[i] for col in cols), lam, channel_skip=True, per_channel=True, channel_weights=cw_d[i],
                                     position_weights=off)
            else:
                off = misaligned(cols[0][i])
                assert F.form_of_one(off, *(col[i] for col in cols[1:]), pos_w=False) == (1, linear)
                s = gmc.quantize_rdo(off, *(col[i] for col in cols[1:]), lam, channel_skip=True, per_channel=True)
            assert skey(s) == skey(got[i]), (lam, i)
        # stacked tensors: the two seeds of one shape as [2, ...] tensors
        for k in range(len(Q.SHAPES)):
            skw = dict(channel_weights=cw_d[2 * k], position_weights=torch.stack([pw_d[2 * k], pw_d[2 * k + 1]])[:, None]) if weighted else {}
            st = gmc.quantize_rdo_batch(*(torch.cat(col[2 * k:2 * k + 2]) for col in cols), lam, channel_skip=True, per_channel=True, **skw)
            assert [skey(s) for s in st] == [skey(g) for g in got[2 * k:2 * k + 2]], (lam, k)
    assert any_skipped
    # without per_channel: no flags, the same sums
    q = gmc.quantize_rdo(*(col[2] for col in cols), 0.5, channel_skip=True, channel_weights=cw_d[2] if weighted else None,
                         position_weights=pw_d[2] if weighted else None)
    r = S.rdoq(oracle, L, mode, *cases[2], 0.5, clamp=clamp, cw=cws[2] if weighted else None, pw=pws[2] if weighted else None, priced=priced[2])
    assert q.skipped is None and q.channel_bits_q_after is None
    check(q, r, "no per_channel")


@pytest.mark.parametrize("mode", MODES)
def test_skip_with_fp16_planes_and_logits(oracle, mode):
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    y, s, m, w = T.make_latent(21, 32, 16, 8, clamp=False, zero_frac=0.2)
    cw, pw = W.chan_w(32), W.pos_w(128).reshape(16, 8)
    p16 = T.to_float16_planes(s, m, w)
    wide = [a.astype(np.float32) for a in p16]
    for kwr, kwg in ((dict(), dict()), (dict(cw=cw, pw=pw), dict(channel_weights=dv(cw), position_weights=dv(pw)))):
        ref = S.rdoq(oracle, L, mode, y, *wide, 0.5, **kwr)
        assert ref["n_skipped"] > 0
        check(gmc.quantize_rdo(dv(y), *(dv(a) for a in p16), 0.5, per_channel=True, channel_skip=True, **kwg), ref, "fp16")
        c = gmc.rd_curve(dv(y), *(dv(a) for a in p16), [0.5], channel_skip=True, **kwg)
        assert (c.bits_q_after[0], c.n_changed[0], c.ddist_q[0], c.n_skipped[0]) == (ref["bits_q_after"], ref["n_changed"], ref["ddist_q"], ref["n_skipped"])
    # logits: the reference gets the weights the kernels' own softmax over K makes of them
    M, hw = 32, 128
    lg = np.log(w).astype(np.float32)
    rows = dv(lg.reshape(4, M * hw).T)
    pi_d = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), pi_d.data_ptr(), M * hw))
    pi = np.ascontiguousarray(pi_d.cpu().numpy().T).reshape(1, 4 * M, 16, 8)
    ref = S.rdoq(oracle, L, mode, y, s, m, pi, 0.5, cw=cw, pw=pw)
    check(gmc.quantize_rdo(dv(y), dv(s), dv(m), dv(lg), 0.5, weights_are_logits=True, per_channel=True, channel_skip=True, channel_weights=dv(cw),
                           position_weights=dv(pw)), ref, "logits")


# ---- 2. without skipping: today's results, through both boundaries -------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_default_and_a_null_skip_array_change_nothing(mode, monkeypatch):
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    cases = make_cases(True)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    cw_d = [dv(W.chan_w(c[0].shape[1])) for c in cases]
    budgets = [V.budget_of(c.nbytes[0], c.nbytes[-1]) for c in gmc.rd_curve_batch(*cols, [0.0, 16.0])]
    want = None
    for native in (True, False):
        if not native:
            monkeypatch.setattr(_lib, "native", lambda: None)  # the ctypes boundary
        for kw in (dict(), dict(channel_weights=cw_d)):
            got = ([key(q) for q in gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True, **kw)],
                   [ckey(c) for c in gmc.rd_curve_batch(*cols, LAMBDAS16, **kw)],
                   [bkey(q) for q in gmc.quantize_to_budget_batch(*cols, budgets, per_channel=True, **kw)])
            off = ([key(q) for q in gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True, channel_skip=False, **kw)],
                   [ckey(c) for c in gmc.rd_curve_batch(*cols, LAMBDAS16, channel_skip=False, **kw)],
                   [bkey(q) for q in gmc.quantize_to_budget_batch(*cols, budgets, per_channel=True, channel_skip=False, **kw)])
            assert got == off
            if not kw:
                want = want or got
                assert got == want  # both boundaries
        q = gmc.quantize_rdo_batch(*cols, 0.5)[0]
        assert type(q) is RdoQuantized and (q.n_skipped, q.n_eligible, q.skipped) == (None, None, None)
        assert gmc.rd_curve_batch(*cols, [0.5])[0].n_skipped is None and gmc.quantize_to_budget_batch(*cols, budgets)[0].n_skipped is None
    # the C entry points: the _w forms are the _s forms with NULL
    Lb = _lib.lib()
    y, s, m, w = (col[2] for col in cols)

    def item(struct=_lib.fgmm_rdoq_item):
        it = struct()
        out = torch.empty_like(y)
        it.y = y.data_ptr()
        if struct is _lib.fgmm_rdoq_item:
            it.y_rdo = out.data_ptr()
        it.params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), 32 * 128, 128, _lib.FGMM_F32, 0)
        it.M, it.K, it.hw = 32, 4, 128
        return it, out

    torch.cuda.synchronize()
    (a, ya), (b, yb) = item(), item()
    assert Lb.fgmm_gmc_rdoq_batch_w(_lib.ctx(0), None, a, 1, gmc._mode(), 1, 0.5, None) == 0
    assert Lb.fgmm_gmc_rdoq_batch_s(_lib.ctx(0), None, b, 1, gmc._mode(), 1, 0.5, None, None) == 0
    outs = lambda it: (it.n_changed, it.bits_q_before, it.bits_q_after, it.abs_max, it.status)  # noqa: E731
    assert torch.equal(yb, ya) and outs(b) == outs(a) and a.n_changed > 0
    (a, _), (b, _) = item(_lib.fgmm_rdcurve_item), item(_lib.fgmm_rdcurve_item)
    lams = (C.c_double * 16)(*LAMBDAS16)
    assert Lb.fgmm_gmc_rdcurve_batch_w(_lib.ctx(0), None, a, 1, gmc._mode(), 1, lams, 16, None) == 0
    assert Lb.fgmm_gmc_rdcurve_batch_s(_lib.ctx(0), None, b, 1, gmc._mode(), 1, lams, 16, None, None) == 0
    assert bytes(a) == bytes(b) and a.n_changed[7] > 0
    (a, ya), (b, yb) = item(), item()
    ra, rb, bud = _lib.fgmm_budget_result(), _lib.fgmm_budget_result(), (C.c_uint64 * 1)(budgets[2])
    assert Lb.fgmm_gmc_rdoq_budget_batch_w(_lib.ctx(0), None, a, 1, gmc._mode(), 1, None, 1, bud, 16.0, 2, ra, None) == 0
    assert Lb.fgmm_gmc_rdoq_budget_batch_s(_lib.ctx(0), None, b, 1, gmc._mode(), 1, None, 1, bud, 16.0, 2, rb, None, None) == 0
    assert torch.equal(yb, ya) and outs(b) == outs(a) and bytes(ra) == bytes(rb) and 0.0 < ra.lambda_ < 16.0


# ---- 3. the curve with channel skipping -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_skip_curve_against_the_reference_and_against_quantize_rdo(oracle, mode, clamp, weighted):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases, cws, pws, priced, wts, ones, hws = priced_cases(oracle, mode, clamp)
    n8 = len(cases) - 1
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    cw_d, pw_d = [dv(a) for a in cws], [dv(a) for a in pws]

    def kw(sel):
        return dict(channel_skip=True, channel_weights=[cw_d[i] for i in sel], position_weights=[pw_d[i] for i in sel]) if weighted else dict(channel_skip=True)

    refs = [S.curve(p, LAMBDAS16, wt, hw) for p, wt, hw in zip(priced, wts if weighted else ones, hws)]
    got = gmc.rd_curve_batch(*(col[:n8] for col in cols), LAMBDAS16, **kw(range(n8))) + gmc.rd_curve_batch(*(col[n8:] for col in cols), LAMBDAS16, **kw([n8]))
    plain = gmc.rd_curve_batch(*(col[:n8] for col in cols), LAMBDAS16, **{k: v for k, v in kw(range(n8)).items() if k != "channel_skip"})
    for i, (g, r) in enumerate(zip(got, refs)):
        assert isinstance(g, RdCurve) and g.bits_q_before == r["bits_q_before"], i
        assert (list(g.bits_q_after), list(g.n_changed), list(g.ddist_q), list(g.n_skipped)) == (r["bits_q_after"], r["n_changed"], r["ddist_q"], r["n_skipped"]), i
        assert (g.bits_q_after[0], g.n_changed[0], g.ddist_q[0], g.n_skipped[0]) == (g.bits_q_before, 0, 0, 0)  # lambda = 0
        assert max(g.n_skipped) > 0, i
        assert g.n_eligible == r["n_eligible"], i
    for g, u in zip(got, plain):
        assert all(a <= b for a, b in zip(g.bits_q_after, u.bits_q_after)) and g.bits_q_after != u.bits_q_after and g.n_symbols == u.n_symbols
    # each point is quantize_rdo(channel_skip=True) at that lambda: a cross-check that needs no reference
    for j, lam in enumerate(LAMBDAS16):
        qs = gmc.quantize_rdo_batch(*(col[:n8] for col in cols), lam, **kw(range(n8))) + gmc.quantize_rdo_batch(*(col[n8:] for col in cols), lam, **kw([n8]))
        for g, q in zip(got, qs):
            assert (g.bits_q_before, g.bits_q_after[j], g.n_changed[j], g.ddist_q[j], g.n_skipped[j], g.n_eligible) == (
                q.bits_q_before, q.bits_q_after, q.n_changed, q.ddist_q, q.n_skipped, q.n_eligible), (j, lam)
    # a single call on the 1-wide path, 17 lambdas (two chunks), the same bits on every run
    for i in (0, 3, 6, n8):
        off = misaligned(cols[0][i])
        assert F.form_of_one(off, *(col[i] for col in cols[1:]), pos_w=pw_d[i] if weighted else False) == (1, hws[i] % 64 == 0)
        one = gmc.rd_curve(off, *(col[i] for col in cols[1:]), LAMBDAS16, channel_skip=True,
                           channel_weights=cw_d[i] if weighted else None, position_weights=pw_d[i] if weighted else None)
        assert ckey(one) + (one.n_skipped, one.n_eligible) == ckey(got[i]) + (got[i].n_skipped, got[i].n_eligible), i
    more = gmc.rd_curve_batch(*(col[:n8] for col in cols), LAMBDAS16 + [0.4], **kw(range(n8)))
    assert [c.n_skipped[:16] for c in more] == [g.n_skipped for g in got[:n8]] and all(len(c.n_skipped) == 17 for c in more)


# ---- 4. the budget search with channel skipping ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_skip_budget_against_the_reference_search(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases = V.budget_cases(clamp)
    cws = [W.chan_w(c[0].shape[1]) for c in cases]
    pws = [W.pos_w(c[0].shape[2] * c[0].shape[3]).reshape(c[0].shape[2:]) for c in cases]
    hws = [c[0].shape[2] * c[0].shape[3] for c in cases]
    priced = [V.price(oracle, L, mode, *c, clamp=clamp) for c in cases]
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    ids = [i % 3 for i in range(len(cases))]  # three groups, ids interleaved
    members = [[i for i in range(len(cases)) if ids[i] == g] for g in range(3)]
    for weighted in (False, True):
        wts = [W.weights_of(*c, cw, pw, clamp=clamp) if weighted else W.weights_of(*c, clamp=clamp) for c, cw, pw in zip(cases, cws, pws)]
        kw = dict(channel_weights=[dv(a) for a in cws], position_weights=[dv(a) for a in pws]) if weighted else {}
        rkw = [dict(cw=cw, pw=pw) if weighted else {} for cw, pw in zip(cws, pws)]
        fs = [S.group_f(L, [priced[i] for i in mem], [wts[i] for i in mem], [hws[i] for i in mem]) for mem in members]
        plain_fs = [W.group_f(L, [priced[i] for i in mem], [wts[i] for i in mem]) for mem in members]
        budgets = [V.budget_of(*f([0.0, 16.0])) for f in plain_fs]  # the budgets of the plain search's tests
        wants = [V.search(f, b) for f, b in zip(fs, budgets)]
        plain = [V.search(f, b) for f, b in zip(plain_fs, budgets)]
        assert all(0.0 < w["lam"] <= u["lam"] and w["status"] == 0 for w, u in zip(wants, plain))
        assert any(w["lam"] < u["lam"] for w, u in zip(wants, plain))  # (skipping is not idle in the search)
        got = gmc.quantize_to_budget_batch(*cols, budgets, groups=ids, per_channel=True, channel_skip=True, **kw)
        for i, g in enumerate(got):
            want = wants[ids[i]]
            assert isinstance(g, BudgetQuantized)
            assert (g.lam, g.bytes_pred, g.passes, g.budget_met) == (want["lam"], want["bytes_pred"], want["passes"], True), (i, g, want)
            check(g, S.rdoq(oracle, L, mode, *cases[i], want["lam"], clamp=clamp, priced=priced[i], **rkw[i]), i)
        for gi, mem in enumerate(members):
            assert sum(V.stream_bytes(L, got[i].bits_q_after) for i in mem) == wants[gi]["bytes_pred"] <= budgets[gi]
    # every item its own group, refine = 0; a single call; a budget nothing meets
    own = [S.group_f(L, [p], [wt], [hw]) for p, wt, hw in zip(priced, wts, hws)]
    b1 = [V.budget_of(*f([0.0, 16.0])) for f in own]
    for i, g in enumerate(gmc.quantize_to_budget_batch(*cols, b1, refine=0, channel_skip=True, **kw)):
        want = V.search(own[i], b1[i], refine=0)
        assert (g.lam, g.bytes_pred, g.passes) == (want["lam"], want["bytes_pred"], 1) and g.bytes_pred <= b1[i], i
    i = 5
    one = gmc.quantize_to_budget(*(col[i] for col in cols), b1[i], channel_skip=True, channel_weights=kw["channel_weights"][i],
                                 position_weights=kw["position_weights"][i])
    want = V.search(own[i], b1[i])
    assert (one.lam, one.bytes_pred, one.passes) == (want["lam"], want["bytes_pred"], want["passes"])
    unmet = gmc.quantize_to_budget(*(col[i] for col in cols), 0, channel_skip=True)
    want = V.search(S.group_f(L, [priced[i]], [W.weights_of(*cases[i], clamp=clamp)], [hws[i]]), 0)
    assert (unmet.lam, unmet.bytes_pred, unmet.budget_met) == (16.0, want["bytes_pred"], False) and want["status"] == V.BUDGET_UNMET


# ---- 5. the invariant: y_rdo prices and codes to exactly what the call reported -----------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_the_estimate_of_the_result_is_its_bits_after_and_it_round_trips(mode):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    cases = make_cases(True)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    for lam in (0.5, 5.0):
        qs = gmc.quantize_rdo_batch(*cols, lam, channel_skip=True)
        ests = gmc.estimate_bits_batch([q.y for q in qs], *cols[1:])
        for i, (q, e) in enumerate(zip(qs, ests)):
            assert e.bits_q == q.bits_q_after and e.zero_bitmap.tolist() == q.zero_bitmap.tolist() and e.abs_max == q.abs_max, (lam, i)
            (b, am, zb), yq = gmc.compress(q.y, *(col[i] for col in cols[1:]))
            assert len(b) - V.stream_bytes(L, q.bits_q_after) in (0, 4), (lam, i, len(b))
            assert (am, zb.cpu().tolist()) == (q.abs_max, q.zero_bitmap.tolist())
            assert torch.equal(yq, q.y) and torch.equal(gmc.decompress(b, am, zb, *(col[i] for col in cols[1:])), q.y), (lam, i)
        assert any(q.n_skipped > 0 for q in qs)


# ---- 6. edges ---------------------------------------------------------------------------------------------------------------------------
def test_edges(oracle):
    """A channel holding one NaN and one holding one inf are kept, the latent with them; 15.4 against 15.6 as a channel's maximum lies on
    either side of FGMM_SKIP_VMAX; a channel with a single non-zero latent at small lambda; an item with no coded channel; M * hw == 0;
    a zero chan_w on a coded channel, skipped at any lambda > 0.  The ``nzA == 0`` clause of the rule is decisive only on rounding ties
    (an emptied channel has Dk == Dz up to the two roundings, and lam_q * A > 0): it is covered through the reference in the sweeps
    above, not by a constructed case."""
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    M, h, w = 8, 8, 13
    y, s, m, pi = T.make_latent(31, M, h, w, clamp=False)
    y = (y * np.float32(0.02)).astype(np.float32)  # faint: every |y| < 0.5 but what is set below
    assert np.abs(y).max() < 0.49
    s[:] = np.float32(0.4)
    m[:] = np.float32(0.0)
    y[0, 0, 0, 0] = np.nan
    y[0, 1, 2, 3], y[0, 1, 0, 0] = np.inf, 1.2
    y[0, 2, 1, 1], y[0, 2, 4, 4] = 15.4, 0.6  # round(15.4) = 15: eligible
    y[0, 3, 1, 1], y[0, 3, 4, 4] = 15.6, 0.6  # round(15.6) = 16: never skipped
    y[0, 4, 7, 12] = 0.9  # a single non-zero latent
    y[0, 5, 3, 3], y[0, 5, 3, 4] = -0.7, 0.9  # (channel 5 also carries the zero chan_w below)
    y[0, 6, 0, 5] = 2.4
    t = [dv(a) for a in (y, s, m, pi)]
    for lam in (1e-6, 1e-3, 0.5, 5.0):
        ref = S.rdoq(oracle, L, "polya", y, s, m, pi, lam)
        q = gmc.quantize_rdo(*t, lam, channel_skip=True, per_channel=True)
        check(q, ref, lam)
        got = q.y.cpu().numpy()
        assert np.isnan(got[0, 0, 0, 0]) and got[0, 1, 2, 3] == np.inf and not q.skipped[0] and not q.skipped[1]
        assert not q.skipped[3] and got[0, 3, 1, 1] in (15.0, 16.0, 17.0) and not q.skipped[7] and q.zero_bitmap[7] == 0
        assert q.n_eligible == 4  # channels 2, 4, 5, 6
        c = gmc.rd_curve(*t, [lam], channel_skip=True)
        assert (c.bits_q_after[0], c.n_changed[0], c.ddist_q[0], c.n_skipped[0]) == (q.bits_q_after, q.n_changed, q.ddist_q, q.n_skipped)
    assert ref["skipped"][2] and ref["skipped"][4]  # at lambda = 5 the faint eligible channels go, 15 and all
    small = gmc.quantize_rdo(*t, 1e-6, channel_skip=True, per_channel=True)
    assert not small.skipped[4] and small.y[0, 4, 7, 12] == 1.0  # a single non-zero latent at small lambda stays
    # a zero chan_w on a coded channel: Jz = 0 < Jk at any lambda > 0
    cw = np.ones(M, np.float32)
    cw[5] = 0.0
    for lam in (1e-3, 0.5):
        ref = S.rdoq(oracle, L, "polya", y, s, m, pi, lam, cw=cw)
        q = gmc.quantize_rdo(*t, lam, channel_skip=True, per_channel=True, channel_weights=dv(cw))
        check(q, ref, ("zero chan_w", lam))
        assert q.skipped[5] and not q.y[0, 5].any()
    # an item with no coded channel, beside one with; M * hw == 0
    dead = [dv(a) for a in T.make_latent(32, 4, 4, 4)]
    dead[0] = dead[0] * 0.01
    qs = gmc.quantize_rdo_batch([dead[0], t[0]], [dead[1], t[1]], [dead[2], t[2]], [dead[3], t[3]], 0.5, channel_skip=True, per_channel=True)
    assert (qs[0].n_skipped, qs[0].n_eligible, qs[0].ddist_q, qs[0].bits_q_after, qs[0].n_changed) == (0, 0, 0, 0, 0) and not qs[0].y.any()
    assert not qs[0].skipped.any() and skey(qs[1]) == skey(gmc.quantize_rdo(*t, 0.5, channel_skip=True, per_channel=True))
    cs = gmc.rd_curve_batch([dead[0], t[0]], [dead[1], t[1]], [dead[2], t[2]], [dead[3], t[3]], [0.5], channel_skip=True)
    assert (cs[0].bits_q_after, cs[0].n_skipped) == ((0,), (0,)) and cs[1].n_skipped == (qs[1].n_skipped,)
    empty = [torch.zeros((1, 0, 4, 4), device=DEV), torch.zeros((1, 0, 4, 4), device=DEV), torch.zeros((1, 0, 4, 4), device=DEV), torch.zeros((1, 0, 4, 4), device=DEV)]
    e = gmc.quantize_rdo(*empty, 0.5, channel_skip=True, per_channel=True)
    assert (e.n_skipped, e.n_eligible, e.ddist_q, e.bits_q_after) == (0, 0, 0, 0) and e.skipped.numel() == 0


# ---- 7. the latent codecs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_codecs_with_channel_skipping(mode):
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    # the latent codec alone: y_hat is the skip-quantised latent, the stream decodes to it and is no longer than without skipping
    y, s, m, w = (dv(a) for a in T.make_latent(4, 32, 16, 8, zero_frac=0.5))
    lg = torch.log(w)
    params = torch.cat([s, m, lg], 1)
    on = GaussianMixtureConditionalLatentCodec(K=4, mode=mode, rdo_lambda=0.5, rdo_channel_skip=True).cuda()
    off = GaussianMixtureConditionalLatentCodec(K=4, mode=mode, rdo_lambda=0.5).cuda()
    a, b = on.compress(y, params), off.compress(y, params)
    _, sc, me, we = on.coder_inputs_rdo(y, params, 0.0)
    q = on.gaussian_mixture_conditional.quantize_rdo(y, sc, me, we, 0.5, channel_skip=True)
    assert q.n_skipped > 0 and torch.equal(a["y_hat"], q.y) and not torch.equal(a["y_hat"], b["y_hat"])
    assert torch.equal(off.decompress(a["strings"], a["shape"], params)["y_hat"], q.y)
    assert sum(len(x[0]) for x in a["strings"]) <= sum(len(x[0]) for x in b["strings"])
    bud = GaussianMixtureConditionalLatentCodec(K=4, mode=mode, target_bytes=200, rdo_channel_skip=True).cuda()
    assert torch.equal(bud.coder_inputs(y, params)[0], on.gaussian_mixture_conditional.quantize_to_budget(y, sc, me, we, 200, channel_skip=True).y)
    # the checkerboard codec: the outer setting replaces the inner codec's, as rdo_lambda does
    Ctx, Par = T.exact_modules()
    for seed, c, c_side, h, wd, dead, parity in ((11, 6, 8, 8, 12, 0, "even"), (12, 5, 6, 6, 10, 1, "odd")):
        yy, side = T.exact_codec_inputs(seed, c, c_side, h, wd, dead=dead)
        yy = (yy * np.float32(0.25)).astype(np.float32)  # faint channels: something to skip

        def make(inner_skip=False, **kw):
            return CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, quantizer="noise", mode=mode, rdo_channel_skip=inner_skip)},
                                           context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c), anchor_parity=parity, **kw).cuda()

        codec = make(rdo_lambda=0.5, rdo_channel_skip=True)
        enc = codec.compress(dv(yy), dv(side))
        inner, gmc = codec.latent_codec["y"], codec.latent_codec["y"].gaussian_mixture_conditional
        y_, side_ = codec.unembed(dv(yy)), codec.unembed(dv(side))
        y_hat_ = side_.new_zeros((2, 1, c, h, wd // 2))
        n_skipped = 0
        for i in range(2):
            params_i = codec.entropy_parameters(codec.merge(codec._ctx(y_hat_, i), side_[i]))
            _, sc, me, we = inner.coder_inputs_rdo(y_[i], params_i, 0.0)
            q = gmc.quantize_rdo(y_[i], sc, me, we, 0.5, channel_skip=True)
            y_hat_[i] = q.y
            n_skipped += q.n_skipped
        assert n_skipped > 0 and torch.equal(codec.embed(y_hat_), enc["y_hat"]), seed
        assert torch.equal(make().decompress(enc["strings"], enc["shape"], dv(side))["y_hat"], enc["y_hat"]), seed
        plain = make(rdo_lambda=0.5).compress(dv(yy), dv(side))
        assert sum(len(x[0]) for x in enc["strings"]) <= sum(len(x[0]) for x in plain["strings"]), seed
        # the outer False replaces an inner True; with the outer lambda 0 the inner codec's own settings apply (none: plain rounding)
        assert torch.equal(make(inner_skip=True, rdo_lambda=0.5).compress(dv(yy), dv(side))["y_hat"], plain["y_hat"])
        assert torch.equal(make(inner_skip=True).compress(dv(yy), dv(side))["y_hat"], make().compress(dv(yy), dv(side))["y_hat"])
