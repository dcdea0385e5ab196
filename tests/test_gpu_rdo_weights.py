"""GPU (-m gpu): the weighted distortion of RDOQ, the curve and the budget search (include/flashgmm_amd.h section 3e; the weighted
instantiations of rdoq_kernel and rdcurve_kernel, the domain check beside the census) against tests/rdo_weights_ref.py.  Every output is
compared for EQUALITY: the chosen latents bit for bit, the counts and the integer sums.  The fixed test weights are
``chan_w[c] = (0.25, 1, 4)[c % 3]`` and ``pos_w[p] = (0.5, 1, 2, 1)[p % 4]``; that they change the decisions in every case (at
lambda = 0.5 on at least 3 % of the coded latents, in both directions, each array on its own) is checked on the CPU by
tests/test_rdo_weights_cpu.py.  All shapes are those of tests/rdoq_ref.SHAPES."""
import numpy as np
import pytest
import torch

from flashgmm_amd import BudgetQuantized, GaussianMixtureConditional, RdCurve, RdoQuantized, _lib
from tests import enc_ref as F
from tests import rdcurve_ref as V
from tests import rdo_weights_ref as W
from tests import rdoq_ref as Q
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
LAMBDAS16 = [0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 16.0]


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
    if got.channel_bits_q_after is not None:
        assert got.channel_bits_q_after.tolist() == ref["chan_after"].tolist(), name


def key(q):
    return (q.y.cpu().numpy().tobytes(), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, q.zero_bitmap.tolist(),
            None if q.channel_bits_q_after is None else q.channel_bits_q_after.tolist())


def bkey(q):
    return key(q) + (q.lam, q.bytes_pred, q.budget_met, q.passes)


def ckey(c):
    return (c.lambdas, c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q, c.n_symbols)


def make_cases(clamp):
    return [T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf) for shape in Q.SHAPES for seed, zf in Q.SEEDS]


_PRICED = {}


def priced_cases(oracle, mode, clamp):
    """the sweep's eight cases, their fixed weights and their candidates priced - once per (mode, clamp), shared by the tests"""
    k = (mode, clamp)
    if k not in _PRICED:
        cases = make_cases(clamp)
        cws = [W.chan_w(c[0].shape[1]) for c in cases]
        pws = [W.pos_w(c[0].shape[2] * c[0].shape[3]).reshape(c[0].shape[2:]) for c in cases]
        priced = [V.price(oracle, _lib.lib(), mode, *c, clamp=clamp) for c in cases]
        wts = [W.weights_of(*c, cw, pw, clamp=clamp) for c, cw, pw in zip(cases, cws, pws)]
        _PRICED[k] = (cases, cws, pws, priced, wts)
    return _PRICED[k]


# ---- 1. quantize_rdo with weights ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_weighted_quantize_rdo_against_the_reference(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases, cws, pws, priced, _ = priced_cases(oracle, mode, clamp)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    cw_d, pw_d = [dv(a) for a in cws], [dv(a) for a in pws]
    for lam in Q.LAMBDAS:
        refs = [W.rdoq(oracle, L, mode, *c, lam, clamp=clamp, cw=cw, pw=pw, priced=p) for c, cw, pw, p in zip(cases, cws, pws, priced)]
        got = gmc.quantize_rdo_batch(*cols, lam, per_channel=True, channel_weights=cw_d, position_weights=pw_d)  # mixed shapes
        assert len(got) == len(cases)
        for i, (g, r) in enumerate(zip(got, refs)):
            check(g, r, (lam, i))
            if lam == 0.0:
                assert g.n_changed == 0 and g.bits_q_after == g.bits_q_before
        # single calls (each shape on its own grid); position_weights as [h, w] and as [1, 1, h, w]
        singles = [gmc.quantize_rdo(*(col[i] for col in cols), lam, per_channel=True, channel_weights=cw_d[i],
                                    position_weights=pw_d[i] if i % 2 else pw_d[i][None, None]) for i in range(len(cases))]
        assert [key(s) for s in singles] == [key(g) for g in got], lam
        # a pos_w that is not 16-byte aligned sends the call down the 1-wide path (every shape here is 4-wide otherwise): hw = 128 and
        # hw = 256 on the linear grid, hw = 104 on the tiled one
        for i, aligned, form in ((3, (4, F.TILED), (1, F.LIN)), (4, (4, F.TILED), (1, F.TILED)), (6, (4, F.LIN), (1, F.LIN))):
            off = misaligned(pw_d[i])
            assert F.form_of_one(*(col[i] for col in cols), pos_w=pw_d[i]) == aligned and F.form_of_one(*(col[i] for col in cols), pos_w=off) == form
            s = gmc.quantize_rdo(*(col[i] for col in cols), lam, per_channel=True, channel_weights=cw_d[i], position_weights=off)
            assert key(s) == key(got[i]), (lam, i)
        # stacked tensors: the two seeds of one shape as [2, ...] tensors, a shared [M] and an [N, 1, h, w]
        for k in range(len(Q.SHAPES)):
            st = gmc.quantize_rdo_batch(*(torch.cat(col[2 * k:2 * k + 2]) for col in cols), lam, per_channel=True, channel_weights=cw_d[2 * k],
                                        position_weights=torch.stack([pw_d[2 * k], pw_d[2 * k + 1]])[:, None])
            assert [key(s) for s in st] == [key(g) for g in got[2 * k:2 * k + 2]], (lam, k)
    # one array alone
    r = W.rdoq(oracle, L, mode, *cases[2], 0.5, clamp=clamp, cw=cws[2], priced=priced[2])
    check(gmc.quantize_rdo(*(col[2] for col in cols), 0.5, per_channel=True, channel_weights=cw_d[2]), r, "chan only")
    r = W.rdoq(oracle, L, mode, *cases[2], 0.5, clamp=clamp, pw=pws[2], priced=priced[2])
    check(gmc.quantize_rdo(*(col[2] for col in cols), 0.5, per_channel=True, position_weights=pw_d[2]), r, "pos only")


# ---- 2. without weights: today's results --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_no_weights_none_entries_and_ones_change_nothing(mode, monkeypatch):
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    cases = make_cases(True)
    N = len(cases)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    ones_c = [torch.ones(c[0].shape[1], device=DEV) for c in cases]
    ones_p = [torch.ones(c[0].shape[2:], device=DEV) for c in cases]
    forms = [dict(channel_weights=None, position_weights=None), dict(channel_weights=[None] * N, position_weights=[None] * N),
             dict(channel_weights=ones_c, position_weights=ones_p), dict(channel_weights=ones_c), dict(position_weights=ones_p),
             dict(channel_weights=[o if i % 2 else None for i, o in enumerate(ones_c)], position_weights=[None if i % 2 else o for i, o in enumerate(ones_p)])]
    budgets = [V.budget_of(c.nbytes[0], c.nbytes[-1]) for c in gmc.rd_curve_batch(*cols, [0.0, 16.0])]
    for native in (True, False):
        if not native:
            monkeypatch.setattr(_lib, "native", lambda: None)  # the ctypes boundary
        want_q = [key(q) for q in gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True)]
        want_c = [ckey(c) for c in gmc.rd_curve_batch(*cols, LAMBDAS16)]
        want_b = [bkey(q) for q in gmc.quantize_to_budget_batch(*cols, budgets, per_channel=True)]
        assert any(k[1] > 0 for k in want_q) and any(0.0 < k[-4] < 16.0 for k in want_b)
        for kw in forms:
            assert [key(q) for q in gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True, **kw)] == want_q, kw.keys()
            assert [ckey(c) for c in gmc.rd_curve_batch(*cols, LAMBDAS16, **kw)] == want_c, kw.keys()
            assert [bkey(q) for q in gmc.quantize_to_budget_batch(*cols, budgets, per_channel=True, **kw)] == want_b, kw.keys()
    # the unweighted C entry points are the _w forms with w = NULL
    Lb = _lib.lib()
    y, s, m, w = (col[2] for col in cols)

    def item():
        it = _lib.fgmm_rdoq_item()
        out = torch.empty_like(y)
        it.y, it.y_rdo = y.data_ptr(), out.data_ptr()
        it.params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), 32 * 128, 128, _lib.FGMM_F32, 0)
        it.M, it.K, it.hw = 32, 4, 128
        return it, out

    torch.cuda.synchronize()
    (a, ya), (b, yb), (c, yc) = item(), item(), item()
    null = (_lib.fgmm_rdo_weights * 1)()
    assert Lb.fgmm_gmc_rdoq_batch(_lib.ctx(0), None, a, 1, gmc._mode(), 1, 0.5) == 0
    assert Lb.fgmm_gmc_rdoq_batch_w(_lib.ctx(0), None, b, 1, gmc._mode(), 1, 0.5, None) == 0
    assert Lb.fgmm_gmc_rdoq_batch_w(_lib.ctx(0), None, c, 1, gmc._mode(), 1, 0.5, null) == 0
    for it, out in ((b, yb), (c, yc)):
        assert torch.equal(out, ya) and (it.n_changed, it.bits_q_before, it.bits_q_after, it.abs_max) == (a.n_changed, a.bits_q_before, a.bits_q_after, a.abs_max)
    assert a.n_changed > 0


# ---- 3. the curve with weights ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_weighted_curve_against_the_reference(oracle, mode, clamp):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases, cws, pws, priced, wts = priced_cases(oracle, mode, clamp)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    kw = dict(channel_weights=[dv(a) for a in cws], position_weights=[dv(a) for a in pws])
    refs = [W.curve(p, LAMBDAS16, wt) for p, wt in zip(priced, wts)]
    plain = [V.curve(p, LAMBDAS16) for p in priced]
    got = gmc.rd_curve_batch(*cols, LAMBDAS16, **kw)
    for i, (g, r, u) in enumerate(zip(got, refs, plain)):
        assert isinstance(g, RdCurve) and g.bits_q_before == r["bits_q_before"], i
        assert (list(g.bits_q_after), list(g.n_changed), list(g.ddist_q)) == (r["bits_q_after"], r["n_changed"], r["ddist_q"]), i
        assert g.distortion_added == tuple(d / 2.0 ** 32 for d in r["ddist_q"])
        assert (g.bits_q_after[0], g.n_changed[0], g.ddist_q[0]) == (g.bits_q_before, 0, 0)  # lambda = 0
        assert r["ddist_q"] != u["ddist_q"] and r["bits_q_after"] != u["bits_q_after"], i  # (the weights are not idle)
    # each point is quantize_rdo at that lambda
    for j, lam in enumerate(LAMBDAS16):
        for g, q in zip(got, gmc.quantize_rdo_batch(*cols, lam, **kw)):
            assert (g.bits_q_before, g.bits_q_after[j], g.n_changed[j]) == (q.bits_q_before, q.bits_q_after, q.n_changed), (j, lam)
    # single calls, a misaligned pos_w (1-wide), 17 lambdas (two chunks), the same bits on every run
    for i in (0, 3, 6):
        off = misaligned(kw["position_weights"][i])
        assert F.form_of_one(*(col[i] for col in cols), pos_w=off) == (1, i != 0)  # hw = 16 tiled; 128 and 256 fill 1-wide waves: linear
        one = gmc.rd_curve(*(col[i] for col in cols), LAMBDAS16, channel_weights=kw["channel_weights"][i], position_weights=off)
        assert ckey(one) == ckey(got[i]), i
    more = gmc.rd_curve_batch(*cols, LAMBDAS16 + [0.4], **kw)
    assert [ckey(c)[2][:16] for c in more] == [ckey(g)[2] for g in got] and all(len(c.ddist_q) == 17 for c in more)
    assert [ckey(g) for g in gmc.rd_curve_batch(*cols, LAMBDAS16, **kw)] == [ckey(g) for g in got]


# ---- 4. the budget search with weights and groups ---------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_weighted_budget_against_the_reference_search(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases, cws, pws, priced, wts = priced_cases(oracle, mode, clamp)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    kw = dict(channel_weights=[dv(a) for a in cws], position_weights=[dv(a) for a in pws])
    ids = [i % 3 for i in range(len(cases))]  # three groups, ids interleaved
    members = [[i for i in range(len(cases)) if ids[i] == g] for g in range(3)]
    fs = [W.group_f(L, [priced[i] for i in mem], [wts[i] for i in mem]) for mem in members]
    budgets = [V.budget_of(*f([0.0, 16.0])) for f in fs]
    wants = [V.search(f, b) for f, b in zip(fs, budgets)]
    plain = [V.search(V.group_f(L, [priced[i] for i in mem]), b) for mem, b in zip(members, budgets)]
    assert all(0.0 < w["lam"] < 16.0 and w["status"] == 0 for w in wants)
    assert any(w["lam"] != u["lam"] for w, u in zip(wants, plain)), [(w["lam"], u["lam"]) for w, u in zip(wants, plain)]
    got = gmc.quantize_to_budget_batch(*cols, budgets, groups=ids, per_channel=True, **kw)
    for i, g in enumerate(got):
        want = wants[ids[i]]
        assert isinstance(g, BudgetQuantized)
        assert (g.lam, g.bytes_pred, g.passes, g.budget_met) == (want["lam"], want["bytes_pred"], want["passes"], True), (i, g, want)
        q = gmc.quantize_rdo(*(col[i] for col in cols), g.lam, per_channel=True, channel_weights=kw["channel_weights"][i],
                             position_weights=kw["position_weights"][i])
        assert key(q) == key(g), i
        check(g, W.rdoq(oracle, L, mode, *cases[i], want["lam"], clamp=clamp, cw=cws[i], pw=pws[i], priced=priced[i]), i)
    for gi, mem in enumerate(members):
        assert sum(V.stream_bytes(L, got[i].bits_q_after) for i in mem) == wants[gi]["bytes_pred"] <= budgets[gi]
    # every item its own group, refine = 0; a single call
    own = [W.group_f(L, [p], [wt]) for p, wt in zip(priced, wts)]
    b1 = [V.budget_of(*f([0.0, 16.0])) for f in own]
    for i, g in enumerate(gmc.quantize_to_budget_batch(*cols, b1, refine=0, **kw)):
        want = V.search(own[i], b1[i], refine=0)
        assert (g.lam, g.bytes_pred, g.passes) == (want["lam"], want["bytes_pred"], 1), i
    i = 5
    one = gmc.quantize_to_budget(*(col[i] for col in cols), b1[i], channel_weights=kw["channel_weights"][i], position_weights=kw["position_weights"][i])
    want = V.search(own[i], b1[i])
    assert (one.lam, one.bytes_pred, one.passes) == (want["lam"], want["bytes_pred"], want["passes"])


# ---- 5. a zero weight; fp16 planes; logits; end to end ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_zero_weight_fp16_logits_and_end_to_end(oracle, mode):
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    # a zero-weight channel takes the cheapest of its three candidates everywhere, ties to the earlier; -0.0 counts as 0
    case = T.make_latent(3, 12, 8, 13, clamp=False)
    p = V.price(oracle, L, mode, *case)
    cw, pw = W.chan_w(12), W.pos_w(104).reshape(8, 13)
    cw[1] = 0.0
    ref = W.rdoq(oracle, L, mode, *case, 0.5, cw=cw, pw=pw, priced=p)
    t = [dv(a) for a in case]
    q = gmc.quantize_rdo(*t, 0.5, per_channel=True, channel_weights=dv(cw), position_weights=dv(pw))
    check(q, ref, "zero weight")
    zb = T.to_coder_inputs(*case)[5]
    assert zb[1] == 1
    sl = slice(int(zb[:1].sum()) * 104, (int(zb[:1].sum()) + 1) * 104)
    cm, c0, cp = (c[sl].astype(np.int64) for c in p["costs"])
    want = np.where(cp < np.minimum(cm, c0), 1, np.where(cm < c0, -1, 0))
    v0 = p["vs"][1][sl]
    assert p["cand"][sl].all() and np.array_equal(q.y[0, 1].cpu().numpy().reshape(-1), (v0 + want.astype(np.float32)) + np.float32(0.0))
    assert (want != 0).any()
    cw[1] = -0.0
    assert key(gmc.quantize_rdo(*t, 0.5, per_channel=True, channel_weights=dv(cw), position_weights=dv(pw))) == key(q)
    # end to end: compress(q.y) decodes to q.y, and the bytes are the oracle encoder's on the reference's symbols
    sym, s_, m_, w_, am, zb_after, _ = T.to_coder_inputs(ref["y"], *case[1:])
    (b, am_g, zb_g), yq = gmc.compress(q.y, *t[1:])
    assert bytes(b) == oracle.encode_gmm(mode, sym, s_, m_, w_)
    assert (am_g, zb_g.cpu().tolist()) == (am, zb_after.tolist()) == (q.abs_max, q.zero_bitmap.tolist())
    assert torch.equal(yq, q.y) and torch.equal(gmc.decompress(b, am_g, zb_g, *t[1:]), q.y)
    # fp16 planes
    y, s, m, w = T.make_latent(21, 32, 16, 8, clamp=False, zero_frac=0.2)
    cw, pw = W.chan_w(32), W.pos_w(128).reshape(16, 8)
    p16 = T.to_float16_planes(s, m, w)
    wide = [a.astype(np.float32) for a in p16]
    ref = W.rdoq(oracle, L, mode, y, *wide, 0.5, cw=cw, pw=pw)
    plain = Q.rdoq(oracle, L, mode, y, *wide, 0.5)
    assert not Q.same_float_bits(ref["y"], plain["y"])
    check(gmc.quantize_rdo(dv(y), *(dv(a) for a in p16), 0.5, per_channel=True, channel_weights=dv(cw), position_weights=dv(pw)), ref, "fp16")
    # logits: the reference gets the weights the kernels' own softmax over K makes of them
    M, hw = 32, 128
    lg = np.log(w).astype(np.float32)
    rows = dv(lg.reshape(4, M * hw).T)
    pi_d = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), pi_d.data_ptr(), M * hw))
    pi = np.ascontiguousarray(pi_d.cpu().numpy().T).reshape(1, 4 * M, 16, 8)
    ref = W.rdoq(oracle, L, mode, y, s, m, pi, 0.5, cw=cw, pw=pw)
    check(gmc.quantize_rdo(dv(y), dv(s), dv(m), dv(lg), 0.5, weights_are_logits=True, per_channel=True, channel_weights=dv(cw),
                           position_weights=dv(pw)), ref, "logits")


# ---- 6. factors outside the domain --------------------------------------------------------------------------------------------------
def test_bad_factors_fail_the_call_and_name_the_item(oracle):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    c0, c1 = T.make_latent(3, 12, 8, 13), T.make_latent(4, 12, 8, 13, zero_frac=0.5)
    zb1 = T.to_coder_inputs(*c1)[5]
    dead = int(np.nonzero(zb1 == 0)[0][0])  # a channel of item 1 that is not coded
    cols = [[dv(a), dv(b)] for a, b in zip(c0, c1)]
    cw, pw = W.chan_w(12), W.pos_w(104).reshape(8, 13)
    good = dict(channel_weights=[dv(cw), dv(cw)], position_weights=[dv(pw), dv(pw)])
    refs = [W.rdoq(oracle, L, "polya", *c, 0.5, cw=cw, pw=pw) for c in (c0, c1)]

    def valid():
        for g, r in zip(gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True, **good), refs):
            check(g, r, "after a refused call")

    valid()
    for bad in (float("nan"), -1.0, float("inf"), 257.0, -float("inf")):
        cw_bad = cw.copy()
        cw_bad[dead] = bad  # in chan_w of an uncoded channel of item 1
        kw = dict(channel_weights=[dv(cw), dv(cw_bad)], position_weights=good["position_weights"])
        with pytest.raises(RuntimeError, match=r"FGMM_ERR_INVALID.*item 1\b"):
            gmc.quantize_rdo_batch(*cols, 0.5, **kw)
        valid()
        pw_bad = pw.copy()
        pw_bad[-1, -1] = bad  # in pos_w at the last position, on the 1-wide path, of item 0
        kw = dict(channel_weights=good["channel_weights"], position_weights=[misaligned(dv(pw_bad)), dv(pw)])
        assert F.form_of(*cols, pos_w=kw["position_weights"]) == (1, F.TILED)
        with pytest.raises(RuntimeError, match=r"FGMM_ERR_INVALID.*item 0\b"):
            gmc.quantize_rdo_batch(*cols, 0.5, **kw)
        with pytest.raises(RuntimeError, match=r"FGMM_ERR_INVALID.*item 0\b"):
            gmc.rd_curve_batch(*cols, [0.1, 0.5], **kw)
        with pytest.raises(RuntimeError, match=r"FGMM_ERR_INVALID.*item 0\b"):
            gmc.quantize_to_budget_batch(*cols, 400, **kw)
        valid()
    # the bounds themselves are inside the domain: 0 and 256
    cw_edge = cw.copy()
    cw_edge[0], cw_edge[1] = 256.0, 0.0
    r = W.rdoq(oracle, L, "polya", *c0, 0.5, cw=cw_edge, pw=pw)
    check(gmc.quantize_rdo(*(col[0] for col in cols), 0.5, per_channel=True, channel_weights=dv(cw_edge), position_weights=dv(pw)), r, "0 and 256")
    # every item's status is the error (latent_call's convention)
    it = (_lib.fgmm_rdoq_item * 1)()
    y, s, m, w = (col[0] for col in cols)
    out = torch.empty_like(y)
    it[0].y, it[0].y_rdo = y.data_ptr(), out.data_ptr()
    it[0].params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), 12 * 104, 104, _lib.FGMM_F32, 0)
    it[0].M, it[0].K, it[0].hw = 12, 4, 104
    wd = (_lib.fgmm_rdo_weights * 1)()
    bad_c = dv(np.full(12, 300.0, np.float32))
    wd[0].chan_w = bad_c.data_ptr()
    torch.cuda.synchronize()
    assert L.fgmm_gmc_rdoq_batch_w(_lib.ctx(0), None, it, 1, 0, 1, 0.5, wd) == 1 and it[0].status == 1 and b"item 0" in L.fgmm_last_error()
    valid()


# ---- 7. the latent codecs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_codecs_with_channel_weights_and_importance(mode):
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    Ctx, Par = T.exact_modules()
    for seed, c, c_side, h, w, dead, parity in ((11, 6, 8, 8, 12, 0, "even"), (12, 5, 6, 6, 10, 1, "odd")):
        y, side = T.exact_codec_inputs(seed, c, c_side, h, w, dead=dead)
        cw, imp = dv(W.chan_w(c)), dv(W.pos_w(h * w).reshape(1, 1, h, w))

        def make(weights=None, **kw):
            return CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, quantizer="noise", mode=mode, rdo_channel_weights=weights)},
                                           context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c), anchor_parity=parity, **kw).cuda()

        codec = make(W.chan_w(c), rdo_lambda=0.5)
        assert codec.latent_codec["y"].rdo_channel_weights.is_cuda
        enc = codec.compress(dv(y), dv(side), importance=imp)
        # the same, half by half: the entropy-model calls on the unembedded halves, half i with half i of the map
        inner, gmc = codec.latent_codec["y"], codec.latent_codec["y"].gaussian_mixture_conditional
        y_, side_, imp_ = codec.unembed(dv(y)), codec.unembed(dv(side)), codec.unembed(imp)
        y_hat_ = side_.new_zeros((2, 1, c, h, w // 2))
        strings = []
        for i in range(2):
            params_i = codec.entropy_parameters(codec.merge(codec._ctx(y_hat_, i), side_[i]))
            _, sc, me, we = inner.coder_inputs_rdo(y_[i], params_i, 0.0)
            q = gmc.quantize_rdo(y_[i], sc, me, we, 0.5, channel_weights=cw, position_weights=imp_[i])
            y_hat_[i] = q.y
            strings.append(gmc.compress(q.y, sc, me, we)[0])
            # the inner codec's own entry points hand the map on
            assert torch.equal(inner.coder_inputs_rdo(y_[i], params_i, 0.5, imp_[i])[0], q.y)
            b = gmc.quantize_to_budget(y_[i], sc, me, we, 60, channel_weights=cw, position_weights=imp_[i])
            assert torch.equal(inner.coder_inputs_budget(y_[i], params_i, 60, imp_[i])[0], b.y)
        assert torch.equal(codec.embed(y_hat_), enc["y_hat"]), seed
        assert [bytes(s[0]) for s in enc["strings"]] == [bytes(s[0]) for s in strings], seed
        # the weights are not idle, and each of the two matters
        unweighted = make(rdo_lambda=0.5).compress(dv(y), dv(side))
        only_c = codec.compress(dv(y), dv(side))
        only_p = make(rdo_lambda=0.5).compress(dv(y), dv(side), importance=imp)
        assert len({e["y_hat"].cpu().numpy().tobytes() for e in (enc, unweighted, only_c, only_p)}) == 4, seed
        # an encoder-side choice: a codec built without weights decodes the stream
        dec = make().decompress(enc["strings"], enc["shape"], dv(side))
        assert torch.equal(dec["y_hat"], enc["y_hat"]), seed
        # weights with rdo_lambda == 0 and no target_bytes do nothing
        a, b = make(W.chan_w(c)).compress(dv(y), dv(side), importance=imp), make().compress(dv(y), dv(side))
        assert [bytes(s[0]) for s in a["strings"]] == [bytes(s[0]) for s in b["strings"]] and torch.equal(a["y_hat"], b["y_hat"])
