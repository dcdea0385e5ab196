"""GPU (-m gpu): the rate-distortion curve and quantisation to a byte budget (include/flashgmm_amd.h section 3d; rdcurve_kernel,
flashgmm_amd/csrc/fgmm_rdcurve.hip) against tests/rdcurve_ref.py - the candidates priced once by the oracle's tables and the host's
fgmm_symtab_bits, the decision per lambda in float64, the search restated from the header.  Every comparison is for EQUALITY.  The
conditions that keep the sweep from passing vacuously are checked on the CPU by tests/test_rdcurve_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import BudgetQuantized, GaussianMixtureConditional, RdCurve, _lib
from tests import enc_ref as F
from tests import rdcurve_ref as V
from tests import rdoq_ref as Q
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
LAMBDAS = [0, 0.05, 0.1, 0.5, 5, 0.5, 0.1]  # unsorted, repeated, 0 among them


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ckey(c):
    return (c.lambdas, c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q)


def check_curve(got, ref, lambdas, name):
    assert isinstance(got, RdCurve) and got.lambdas == tuple(float(v) for v in lambdas), name
    assert got.bits_q_before == ref["bits_q_before"], name
    assert (list(got.bits_q_after), list(got.n_changed), list(got.ddist_q)) == (ref["bits_q_after"], ref["n_changed"], ref["ddist_q"]), name
    f = _lib.lib().fgmm_rate_stream_bytes
    assert got.nbytes == tuple(int(f(b)) for b in ref["bits_q_after"]) and got.bits_after == tuple(b / 2.0 ** 24 for b in ref["bits_q_after"])
    assert got.distortion_added == tuple(d / 2.0 ** 32 for d in ref["ddist_q"])


def qkey(q):
    return (q.y.cpu().numpy().tobytes(), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, q.zero_bitmap.tolist())


# ---- (a) the curve against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_curve_against_the_reference(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases = [T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf) for shape in Q.SHAPES for seed, zf in Q.SEEDS]
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    refs = [V.curve(V.price(oracle, L, mode, *c, clamp=clamp), LAMBDAS) for c in cases]
    assert F.form_of(*cols) == (4, F.TILED)  # mixed shapes, every hw a multiple of 4: 4-wide on the tiled grid
    got = gmc.rd_curve_batch(*cols, LAMBDAS)
    assert len(got) == len(cases)
    for i, (g, r) in enumerate(zip(got, refs)):
        check_curve(g, r, LAMBDAS, i)
        assert (g.bits_q_after[0], g.n_changed[0], g.ddist_q[0]) == (g.bits_q_before, 0, 0)  # lambda = 0
    assert any(max(g.n_changed) > 0 for g in got)
    # single calls (each shape on its own grid: 4-wide, tiled at hw = 16, 128 and 104, linear at 256) and stacked [2, ...] tensors agree
    # with the batch
    assert [F.form_of_one(*(col[i] for col in cols), pos_w=False) for i in range(0, len(cases), 2)] == [(4, F.TILED)] * 3 + [(4, F.LIN)]
    singles = [gmc.rd_curve(*(col[i] for col in cols), LAMBDAS) for i in range(len(cases))]
    assert [ckey(s) for s in singles] == [ckey(g) for g in got]
    for k in range(len(Q.SHAPES)):
        st = gmc.rd_curve_batch(*(torch.cat(col[2 * k:2 * k + 2]) for col in cols), LAMBDAS)
        assert [ckey(s) for s in st] == [ckey(g) for g in got[2 * k:2 * k + 2]], k
    # column j is quantize_rdo_batch at lambda_j
    for j, lam in enumerate(LAMBDAS):
        for g, q in zip(got, gmc.quantize_rdo_batch(*cols, lam)):
            assert (g.bits_q_before, g.bits_q_after[j], g.n_changed[j]) == (q.bits_q_before, q.bits_q_after, q.n_changed), (j, lam)
    assert [ckey(g) for g in gmc.rd_curve_batch(*cols, LAMBDAS)] == [ckey(g) for g in got]  # the same bits on every run


# ---- (b) n_lambda limits -----------------------------------------------------------------------------------------------------------------
def test_one_sixteen_and_seventeen_lambdas(oracle):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    case = T.make_latent(3, 12, 8, 13)
    t = [dv(a) for a in case]
    p = V.price(oracle, L, "polya", *case)
    lams = [0.03 * 1.4 ** j for j in range(17)]
    for n in (1, 16, 17):  # 17: two chunks through Python
        check_curve(gmc.rd_curve(*t, lams[:n]), V.curve(p, lams[:n]), lams[:n], n)


# ---- (c) fp16 planes, logits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fp16_planes_and_logits(oracle, mode):
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    y, s, m, w = T.make_latent(21, 32, 16, 8, clamp=False, zero_frac=0.2)
    p16 = T.to_float16_planes(s, m, w)
    ref = V.curve(V.price(oracle, L, mode, y, *(a.astype(np.float32) for a in p16)), LAMBDAS)  # the widened planes
    check_curve(gmc.rd_curve(dv(y), *(dv(a) for a in p16), LAMBDAS), ref, LAMBDAS, "fp16")
    assert max(ref["n_changed"]) > 0
    # logits: the reference gets the weights the kernels' own softmax over K makes of them (fgmm_softmax4_hip, rows (n, 4))
    M, hw = 32, 128
    lg = np.log(w).astype(np.float32)
    rows = dv(lg.reshape(4, M * hw).T)
    pi_d = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), pi_d.data_ptr(), M * hw))
    pi = np.ascontiguousarray(pi_d.cpu().numpy().T).reshape(1, 4 * M, 16, 8)
    ref = V.curve(V.price(oracle, L, mode, y, s, m, pi), LAMBDAS)
    check_curve(gmc.rd_curve(dv(y), dv(s), dv(m), dv(lg), LAMBDAS, weights_are_logits=True), ref, LAMBDAS, "logits")


# ---- (d) edge latents --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_edge_latents(oracle, mode):
    """NaN, +-inf and |y| > 2^20 planted in coded channels: they cost cost(v0) at every lambda and never count as moved"""
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    y, s, m, w = T.make_latent(4, 12, 8, 13)
    y = y.copy()
    zb = T.to_coder_inputs(y, s, m, w)[5]
    coded = np.nonzero(zb)[0]
    vals = [np.nan, np.inf, -np.inf, 2.0 ** 20 + 3, -3e9]
    at = [(int(coded[i % len(coded)]), 3 + i, (2 * i) % 13) for i in range(len(vals))]
    for (c, r, q), v in zip(at, vals):
        y[0, c, r % 8, q] = np.float32(v)
    p = V.price(oracle, L, mode, y, s, m, w)
    assert int((~p["cand"]).sum()) == len(vals)
    ref = V.curve(p, LAMBDAS + [16.0])
    check_curve(gmc.rd_curve(dv(y), dv(s), dv(m), dv(w), LAMBDAS + [16.0]), ref, LAMBDAS + [16.0], "edges")
    n = len(p["yv"])
    assert max(ref["n_changed"]) <= n - len(vals)
    for j, lam in enumerate(LAMBDAS + [16.0]):  # and the RDOQ call itself agrees, planted latents kept
        q = gmc.quantize_rdo(dv(y), dv(s), dv(m), dv(w), lam)
        assert (q.bits_q_after, q.n_changed) == (ref["bits_q_after"][j], ref["n_changed"][j])


# ---- (e) the budget ------------------------------------------------------------------------------------------------------------------------
def check_budget(gmc, got, want, t, lam_args=()):
    """got: the BudgetQuantized of one item; want: the reference search of its group; t: its tensors"""
    assert isinstance(got, BudgetQuantized)
    assert np.float64(got.lam).tobytes() == np.float64(want["lam"]).tobytes(), (got.lam, want["lam"])  # bit for bit
    assert (got.bytes_pred, got.passes, got.budget_met) == (want["bytes_pred"], want["passes"], want["status"] == 0), (got, want)
    q = gmc.quantize_rdo(*t, got.lam, per_channel=True)
    assert qkey(got) == qkey(q) and got.channel_bits_q_after.tolist() == q.channel_bits_q_after.tolist()


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_budget_against_the_reference_search(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases = V.budget_cases(clamp)
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    priced = [V.price(oracle, L, mode, *c, clamp=clamp) for c in cases]
    fs = [V.group_f(L, [p]) for p in priced]
    budgets = [V.budget_of(*f([0.0, 16.0])) for f in fs]
    # every item its own group
    got = gmc.quantize_to_budget_batch(*cols, budgets, per_channel=True)
    for i, (g, f, b) in enumerate(zip(got, fs, budgets)):
        want = V.search(f, b)
        assert 0.0 < want["lam"] < 16.0 and want["moved"] >= 1, i
        check_budget(gmc, g, want, [col[i] for col in cols])
        # end to end: the bytes decode to q.y and are at most 4 over the prediction
        (data, am, zb), yq = gmc.compress(g.y, *(col[i] for col in cols[1:]))
        assert torch.equal(yq, g.y) and torch.equal(gmc.decompress(data, am, zb, *(col[i] for col in cols[1:])), g.y), i
        assert len(bytes(data)) <= g.bytes_pred + 4 and g.bytes_pred <= b, (i, len(bytes(data)), g.bytes_pred, b)
        assert (am, zb.cpu().tolist()) == (g.abs_max, g.zero_bitmap.tolist())
    single = gmc.quantize_to_budget(*(col[3] for col in cols), budgets[3], per_channel=True)
    assert qkey(single) == qkey(got[3]) and (single.lam, single.bytes_pred, single.passes) == (got[3].lam, got[3].bytes_pred, got[3].passes)
    # refine = 0: the round-0 grid's first feasible point
    for i, g in enumerate(gmc.quantize_to_budget_batch(*cols, budgets, refine=0, per_channel=True)):
        want = V.search(fs[i], budgets[i], refine=0)
        assert want["passes"] == 1
        check_budget(gmc, g, want, [col[i] for col in cols])
    # one group of all eight
    f = V.group_f(L, priced)
    b = V.budget_of(*f([0.0, 16.0]))
    want = V.search(f, b)
    got = gmc.quantize_to_budget_batch(*cols, b, groups=[0] * len(cases), per_channel=True)
    assert want["moved"] >= 1 and sum(V.stream_bytes(L, g.bits_q_after) for g in got) == want["bytes_pred"] <= b
    for i, g in enumerate(got):
        check_budget(gmc, g, want, [col[i] for col in cols])
    # two groups with budgets of their own, ids interleaved; the second budget cannot be met (8 bytes), the first is met by round(y)
    ids = [i % 2 for i in range(len(cases))]
    f0, f1 = V.group_f(L, priced[0::2]), V.group_f(L, priced[1::2])
    b0 = f0([0.0])[0]
    got = gmc.quantize_to_budget_batch(*cols, [b0, 8], groups=ids, per_channel=True)
    w0, w1 = V.search(f0, b0), V.search(f1, 8)
    assert (w0["lam"], w0["status"], w0["passes"]) == (0.0, 0, 1) and (w1["lam"], w1["status"], w1["passes"]) == (16.0, V.BUDGET_UNMET, 1)
    for i, g in enumerate(got):
        check_budget(gmc, g, (w0, w1)[ids[i]], [col[i] for col in cols])
        assert g.budget_met == (ids[i] == 0) and (ids[i] == 1 or g.n_changed == 0)


# ---- (f) validation -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_leave_the_context_usable():
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    y, s, m, w = (dv(a) for a in T.make_latent(7, 8, 4, 4))
    want = ckey(gmc.rd_curve(y, s, m, w, [0.5]))

    def curve_item():
        it = _lib.fgmm_rdcurve_item()
        it.y = y.data_ptr()
        it.params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), 8 * 16, 16, _lib.FGMM_F32, 0)
        it.M, it.K, it.hw = 8, 4, 16
        return it

    def rdoq_item(out):
        it = _lib.fgmm_rdoq_item()
        it.y, it.y_rdo = y.data_ptr(), out.data_ptr()
        it.params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), 8 * 16, 16, _lib.FGMM_F32, 0)
        it.M, it.K, it.hw = 8, 4, 16
        return it

    lam17 = (C.c_double * 17)(*([0.5] * 17))
    torch.cuda.synchronize()
    for n in (0, 17):
        assert L.fgmm_gmc_rdcurve_batch(ctx, None, curve_item(), 1, 0, 1, lam17, n) == 1, n
    for bad in (-0.5, float("nan"), float("inf")):
        assert L.fgmm_gmc_rdcurve_batch(ctx, None, curve_item(), 1, 0, 1, (C.c_double * 2)(0.5, bad), 2) == 1, bad
        with pytest.raises((ValueError, RuntimeError)):
            gmc.rd_curve(y, s, m, w, [0.5, bad])
    with pytest.raises((ValueError, RuntimeError)):
        gmc.rd_curve(y, s, m, w, [])
    out, out2 = torch.empty_like(y), torch.empty_like(y)
    arr = (_lib.fgmm_rdoq_item * 2)(rdoq_item(out), rdoq_item(out2))
    res = (_lib.fgmm_budget_result * 2)()
    bud = (C.c_uint64 * 2)(40, 40)

    def budget(groups, n_groups, lambda_max=16.0, refine=2):
        g = None if groups is None else (C.c_int32 * 2)(*groups)
        return L.fgmm_gmc_rdoq_budget_batch(ctx, None, arr, 2, 0, 1, g, n_groups, bud, lambda_max, refine, res)

    for lmax in (0.0, -1.0, float("nan"), float("inf")):
        assert budget(None, 2, lambda_max=lmax) == 1, lmax
        with pytest.raises((ValueError, RuntimeError)):
            gmc.quantize_to_budget(y, s, m, w, 40, lambda_max=lmax)
    assert budget(None, 2, refine=9) == 1 and budget(None, 2, refine=-1) == 1
    with pytest.raises((ValueError, RuntimeError)):
        gmc.quantize_to_budget(y, s, m, w, 40, refine=9)
    assert budget([0, 0], 2) == 1  # group 1 is empty
    assert budget([0, 2], 2) == 1 and budget([-1, 0], 2) == 1  # ids out of range
    assert budget(None, 1) == 1  # without ids every item is its own group
    for groups in ([0, 0, 0], [1, 1], [0, 2]):
        with pytest.raises((ValueError, RuntimeError)):
            gmc.quantize_to_budget_batch([y, y], [s, s], [m, m], [w, w], 40, groups=groups)
    assert budget([0, 1], 2) == 0 and budget(None, 2) == 0  # and the context is usable
    assert ckey(gmc.rd_curve(y, s, m, w, [0.5])) == want
    # an item without latents: zero sums, 8 bytes, any budget >= 8 is met by lambda = 0
    e = torch.empty((1, 0, 4, 4), device=DEV)
    c = gmc.rd_curve(e, e, e, e, [0.0, 0.5])
    assert (c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q, c.nbytes) == (0, (0, 0), (0, 0), (0, 0), (8, 8))
    q = gmc.quantize_to_budget(e, e, e, e, 8)
    assert (q.lam, q.bytes_pred, q.budget_met, q.passes, q.y.numel()) == (0.0, 8, True, 1, 0)


def test_the_ctypes_boundary_gives_the_same(monkeypatch):
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    t = [dv(a) for a in T.make_latent(4, 12, 8, 13, zero_frac=0.5)]
    c, q = gmc.rd_curve(*t, LAMBDAS), gmc.quantize_to_budget(*t, 400)
    monkeypatch.setattr(_lib, "native", lambda: None)
    c2, q2 = gmc.rd_curve(*t, LAMBDAS), gmc.quantize_to_budget(*t, 400)
    assert ckey(c) == ckey(c2) and qkey(q) == qkey(q2) and (q.lam, q.bytes_pred, q.budget_met, q.passes) == (q2.lam, q2.bytes_pred, q2.budget_met, q2.passes)


# ---- (g) the latent codec -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantizer", ["noise", "weighted_mean_ste"])
def test_latent_codec_with_target_bytes(quantizer):
    from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec

    y, s, m, w = T.make_latent(5, 12, 8, 13)
    y, params = dv(y), dv(np.concatenate([s, m, np.log(w)], axis=1))
    plain = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya")
    gmc = plain.gaussian_mixture_conditional
    sc, me, we = plain._params(params)
    d, add = y, None
    if quantizer != "noise":
        add, me = plain._recentre(me, we)
        d = y - add
    at0, at16 = gmc.rd_curve(d, sc, me, we, [0.0, 16.0]).nbytes
    assert at0 == gmc.estimate_bits(d, sc, me, we).nbytes > at16
    target = V.budget_of(at0, at16)  # half way between plain rounding and the default search's largest lambda
    q = gmc.quantize_to_budget(d, sc, me, we, target)
    assert q.budget_met and q.lam > 0 and q.n_changed > 0 and q.bytes_pred <= target
    codec = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya", target_bytes=target)
    enc = codec.compress(y, params)
    (b, am, zb), _ = gmc.compress(q.y, sc, me, we)
    assert torch.equal(enc["y_hat"], q.y) and bytes(enc["strings"][0][0]) == bytes(b) and len(bytes(b)) <= target + 4
    assert torch.equal(plain.coder_inputs_budget(y, params, target)[0], q.y)
    want = q.y if add is None else q.y + add
    for decoder in (codec, plain):  # an encoder-side choice: the decoder needs no switch
        assert torch.equal(decoder.decompress(enc["strings"], enc["shape"], params)["y_hat"], want)
    with pytest.raises(ValueError):
        GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya", target_bytes=target, rdo_lambda=0.5)
    # a codec built without target_bytes returns what it returned before: plain rounding, and RDOQ at its lambda
    a = plain.compress(y, params)
    (b0, _, _), yq0 = gmc.compress(plain.coder_inputs_rdo(y, params, 0.0)[0], sc, me, we)
    assert bytes(a["strings"][0][0]) == bytes(b0) and torch.equal(a["y_hat"], yq0) and bytes(b0) != bytes(b)
    lam = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya", rdo_lambda=0.5)
    assert lam.target_bytes is None and torch.equal(lam.coder_inputs(y, params)[0], gmc.quantize_rdo(d, sc, me, we, 0.5).y)
