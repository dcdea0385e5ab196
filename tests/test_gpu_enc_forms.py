"""GPU (-m gpu): rate_kernel, rdoq_kernel (with rdoq_skip_kernel) and rdcurve_kernel (with its fold kernels) in each of the four launch
forms of their frame (flashgmm_amd/csrc/fgmm_encframe.h) - 1 or 4 positions per lane, the tiled or the linear grid - at the plane sizes
where a form can go wrong: ``tests/enc_ref.ODD_CORPUS``, hw = 1 .. 260, most of them no multiple of 4, with float32, float16 and bfloat16
planes, plain, weighted (include/flashgmm_amd.h section 3e), with channel skipping (3f) and with both.

Every call ASSERTS ITS LAUNCH FORM FIRST, from the tensors it hands over (``enc_ref.form_of``: the launcher's decision restated), and every
comparison is for equality - bytes, integers, float bit patterns - against the oracle's tables priced by the host's ``fgmm_symtab_bits``
(tests/rate_ref.py, rdoq_ref.py, rdcurve_ref.py, rdo_weights_ref.py, rdo_skip_ref.py), fed the widened planes.  That the corpus reaches
every instantiation, that latents move, that channels are skipped and kept in both widths: tests/test_enc_forms_cpu.py."""
import numpy as np
import pytest
import torch

from flashgmm_amd import BudgetQuantized, GaussianMixtureConditional, RdCurve, RdoQuantized, _lib
from tests import enc_ref as F
from tests import rate_ref as R
from tests import rdcurve_ref as V
from tests import rdo_skip_ref as S
from tests import rdo_weights_ref as W
from tests import rdoq_ref as Q
from tests import synth as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N = len(F.ODD_CORPUS)
LAMS16 = list(F.LAMBDAS16)
MODE_CLAMP = [(mode, clamp) for mode in F.MODES for clamp in (True, False)]


# ---- placement ----------------------------------------------------------------------------------------------------------------------------
def dv(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:  # bfloat16 bit patterns
        return torch.from_numpy(a.view(np.int16)).to(DEV).view(torch.bfloat16)
    return torch.from_numpy(a).to(DEV)


def one_in(t):
    """the same values as a dense view one element into a storage of its own (the element before it: NaN)"""
    buf = torch.full((t.numel() + 1,), float("nan"), dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == t.element_size()
    return v


def strided(t):
    """[1, KM, h, w] -> the same values with a channel stride of hw + 2: dense rows in a larger storage, NaN between them"""
    _, KM, h, w = t.shape
    sc = h * w + 2
    buf = torch.full((KM * sc,), float("nan"), dtype=t.dtype, device=t.device)
    v = torch.as_strided(buf, (1, KM, h, w), (KM * sc, sc, w, 1))
    v.copy_(t)
    return v


_PLACED, _PRICED = {}, {}


def placed(clamp, pt):
    """the corpus on the device, each entry placed as ``enc_ref.ODD_CORPUS`` says -> per entry (y, s, m, w, chan_w, pos_w)"""
    if (clamp, pt) not in _PLACED:
        rows = []
        for i, (M, h, w, placement) in enumerate(F.ODD_CORPUS):
            case = F.corpus_case(i, clamp)
            y, planes = dv(case[0]), [dv(a) for a in F.planes_of(case, pt)[0]]
            cw, pw = (dv(a) for a in F.factors(i))
            if placement == "y_off":
                y = one_in(y)
            elif placement == "stride":
                planes = [strided(t) for t in planes]
            elif placement == "pos_w_off":
                pw = one_in(pw)
            rows.append((y, *planes, cw, pw))
        _PLACED[clamp, pt] = rows
    return _PLACED[clamp, pt]


def priced(oracle, mode, clamp, pt):
    """the reference side of every entry, once per (mode, clamp, plane type) -> per entry a dict: ``case`` (y and the widened planes),
    ``p`` (its candidates priced), ``cw`` / ``pw``, ``wt`` (the weights of its coded latents under them), ``ones``, ``hw``"""
    k = (mode, clamp, pt)
    if k not in _PRICED:
        rows = []
        for i, (M, h, w, _) in enumerate(F.ODD_CORPUS):
            case = F.widened_case(i, clamp, pt)
            cw, pw = F.factors(i)
            rows.append(dict(case=case, p=V.price(oracle, _lib.lib(), mode, *case, clamp=clamp), cw=cw, pw=pw, hw=h * w,
                             wt=W.weights_of(*case, cw, pw, clamp=clamp), ones=W.weights_of(*case, clamp=clamp)))
        _PRICED[k] = rows
    return _PRICED[k]


def kwargs(rows, ids, weighted, skip, batch=True):
    kw = dict(channel_skip=True) if skip else {}
    if weighted:
        kw.update(channel_weights=[rows[i][4] for i in ids], position_weights=[rows[i][5] for i in ids])
        if not batch:
            kw.update(channel_weights=kw["channel_weights"][0], position_weights=kw["position_weights"][0])
    return kw


def assert_form(rows, ids, pt, weighted, want=None, outs=None):
    """the form of the call on entries ``ids`` (one call), from the tensors themselves; a single entry: also the planned form"""
    got = F.form_of(*([rows[i][k] for i in ids] for k in range(4)), pos_w=[rows[i][5] for i in ids] if weighted else None, outs=outs)
    if len(ids) == 1:
        assert got == F.planned_form(ids[0], pt, weighted), (ids, pt, weighted, got)
    if want is not None:
        assert got == want, (ids, pt, weighted, got, want)
    return got


def ref_rdoq(oracle, mode, clamp, r, lam, weighted, skip):
    L = _lib.lib()
    kw = dict(cw=r["cw"], pw=r["pw"]) if weighted else {}
    if skip:
        return S.rdoq(oracle, L, mode, *r["case"], lam, clamp=clamp, priced=r["p"], **kw)
    if weighted:
        return W.rdoq(oracle, L, mode, *r["case"], lam, clamp=clamp, priced=r["p"], **kw)
    return Q.rdoq(oracle, L, mode, *r["case"], lam, clamp=clamp)


def ref_curve(r, lams, weighted, skip):
    wt = r["wt"] if weighted else r["ones"]
    if skip:
        return S.curve(r["p"], lams, wt, r["hw"])
    return W.curve(r["p"], lams, wt) if weighted else V.curve(r["p"], lams)


def check(got, ref, skip, name):
    assert isinstance(got, RdoQuantized)
    y = got.y.cpu().numpy()
    assert Q.same_float_bits(y, ref["y"]), (name, int((y.view(np.uint32) != ref["y"].view(np.uint32)).sum()))
    assert (got.n_changed, got.bits_q_before, got.bits_q_after) == (ref["n_changed"], ref["bits_q_before"], ref["bits_q_after"]), name
    assert (got.abs_max, got.zero_bitmap.tolist()) == (ref["abs_max"], list(ref["zero_bitmap"])), name
    assert got.channel_bits_q_after.tolist() == ref["chan_after"].tolist(), name
    if skip:
        assert (got.n_skipped, got.n_eligible, got.ddist_q) == (ref["n_skipped"], ref["n_eligible"], ref["ddist_q"]), name
        assert got.skipped.dtype == torch.bool and got.skipped.tolist() == ref["skipped"].tolist(), name
    else:
        assert (got.n_skipped, got.n_eligible, got.skipped) == (None, None, None), name


def qkey(q):
    return (q.y.cpu().numpy().tobytes(), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, q.zero_bitmap.tolist(),
            None if q.channel_bits_q_after is None else q.channel_bits_q_after.tolist(), q.n_skipped, q.n_eligible, q.ddist_q,
            None if q.skipped is None else q.skipped.tolist())


def ckey(c):
    return (c.lambdas, c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q, c.n_symbols, c.n_skipped, c.n_eligible)


def ekey(e):
    return (e.bits_q, e.nbytes, e.n_symbols, e.n_bypass, e.abs_max, e.zero_bitmap.tolist(), e.channel_bits_q.tolist(), e.latent_bits.cpu().numpy().tobytes())


def ref_rate(oracle, mode, clamp, case):
    """what an estimate must say: the oracle's table of the latent, priced entry by entry by the host function"""
    y = case[0]
    M, hw = y.shape[1], y.shape[2] * y.shape[3]
    sym, s_, m_, w_, am, zb, _ = T.to_coder_inputs(*case, clamp=clamp)
    bits_q, nb, cost = R.host_bits(_lib.lib(), oracle.symtab(mode, sym, s_, m_, w_), sym, costs=True)
    nz = np.nonzero(zb)[0]
    chan, bmap = np.zeros(M, np.int64), np.zeros((M, hw), np.float32)
    chan[nz] = cost.reshape(len(nz), hw).astype(np.int64).sum(1)
    bmap[nz] = cost.reshape(len(nz), hw).astype(np.float32) * np.float32(2.0 ** -24)
    return dict(bits_q=bits_q, n_bypass=nb, n_symbols=len(sym), abs_max=am, zero_bitmap=zb.tolist(), chan=chan, map=bmap)


# ---- 1. the rate ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,clamp", MODE_CLAMP)
def test_rate_in_every_form(oracle, mode, clamp):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    n_bypass = 0
    for pt in F.PLANE_TYPES:
        rows, refs = placed(clamp, pt), priced(oracle, mode, clamp, pt)
        for i in range(N):
            form = assert_form(rows, [i], pt, False)
            e = gmc.estimate_bits(*rows[i][:4], per_channel=True, per_latent=True)
            assert assert_form(rows, [i], pt, False, outs=[e.latent_bits]) == form
            ref = ref_rate(oracle, mode, clamp, refs[i]["case"])
            name = (pt, i, form)
            assert (e.bits_q, e.n_bypass, e.n_symbols) == (ref["bits_q"], ref["n_bypass"], ref["n_symbols"]), name
            assert (e.abs_max, e.zero_bitmap.tolist()) == (ref["abs_max"], ref["zero_bitmap"]), name
            assert e.channel_bits_q.tolist() == ref["chan"].tolist(), name
            assert np.array_equal(e.latent_bits.cpu().numpy().reshape(ref["map"].shape).view(np.uint32), ref["map"].view(np.uint32)), name
            plain = gmc.estimate_bits(*rows[i][:4])  # (no map: the call has no per-latent output)
            assert (plain.bits_q, plain.n_bypass, plain.channel_bits_q, plain.latent_bits) == (e.bits_q, e.n_bypass, None, None), name
            n_bypass += e.n_bypass
    assert n_bypass > 0


# ---- 2. RDOQ --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,clamp", MODE_CLAMP)
def test_rdoq_in_every_form(oracle, mode, clamp):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for pt in F.PLANE_TYPES:
        rows, refs = placed(clamp, pt), priced(oracle, mode, clamp, pt)
        for i in range(N):
            t = rows[i][:4]
            for weighted, skip in F.FORMS4:
                form = assert_form(rows, [i], pt, weighted)
                for lam in F.LAMBDAS3:
                    name = (pt, i, form, weighted, skip, lam)
                    q = gmc.quantize_rdo(*t, lam, per_channel=True, **kwargs(rows, [i], weighted, skip, batch=False))
                    assert assert_form(rows, [i], pt, weighted, outs=[q.y]) == form
                    check(q, ref_rdoq(oracle, mode, clamp, refs[i], lam, weighted, skip), skip, name)
                    if lam == 0.0:
                        assert q.n_changed == 0 and q.bits_q_after == q.bits_q_before and not q.n_skipped, name
                    # the result prices to what the call reported, and codes to bytes that decode to it.  A channel whose last non-zero
                    # latent moved to zero is no longer coded for q.y, while bits_q_after (section 3c) still counts its zeros - at hw = 1
                    # that is the whole item - so without skipping the estimate is bits_q_after less exactly those channels' sums;
                    # with skipping such a channel is skipped (nzA == 0) and counts nothing: plain equality
                    e = gmc.estimate_bits(q.y, *t[1:])
                    still = q.zero_bitmap != 0
                    assert e.bits_q == int(q.channel_bits_q_after[still].sum()) == q.bits_q_after - int(q.channel_bits_q_after[~still].sum()), name
                    assert e.bits_q == q.bits_q_after or not skip, name
                    assert (e.abs_max, e.zero_bitmap.tolist()) == (q.abs_max, q.zero_bitmap.tolist()), name
                    (b, am, zb), yq = gmc.compress(q.y, *t[1:])
                    assert (am, zb.cpu().tolist()) == (q.abs_max, q.zero_bitmap.tolist()), name
                    assert torch.equal(yq, q.y) and torch.equal(gmc.decompress(b, am, zb, *t[1:]), q.y), name


# ---- 3. the curve ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,clamp", MODE_CLAMP)
def test_curve_in_every_form(oracle, mode, clamp):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for pt in F.PLANE_TYPES:
        rows, refs = placed(clamp, pt), priced(oracle, mode, clamp, pt)
        for i in range(N):
            t = rows[i][:4]
            for weighted, skip in F.FORMS4:
                form = assert_form(rows, [i], pt, weighted)
                name = (pt, i, form, weighted, skip)
                kw = kwargs(rows, [i], weighted, skip, batch=False)
                c = gmc.rd_curve(*t, LAMS16, **kw)
                ref = ref_curve(refs[i], LAMS16, weighted, skip)
                assert isinstance(c, RdCurve) and c.bits_q_before == ref["bits_q_before"] and c.n_symbols == len(refs[i]["p"]["yv"]), name
                assert (list(c.bits_q_after), list(c.n_changed), list(c.ddist_q)) == (ref["bits_q_after"], ref["n_changed"], ref["ddist_q"]), name
                if skip:
                    assert (list(c.n_skipped), c.n_eligible) == (ref["n_skipped"], ref["n_eligible"]), name
                else:
                    assert c.n_skipped is None and c.n_eligible is None, name
                for j, lam in enumerate(LAMS16):  # column j is quantize_rdo at lambda j
                    q = gmc.quantize_rdo(*t, lam, **kw)
                    assert (c.bits_q_before, c.bits_q_after[j], c.n_changed[j]) == (q.bits_q_before, q.bits_q_after, q.n_changed), (name, lam)
                    if skip:
                        assert (c.ddist_q[j], c.n_skipped[j], c.n_eligible) == (q.ddist_q, q.n_skipped, q.n_eligible), (name, lam)


# ---- 4. the budget --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,clamp", MODE_CLAMP)
def test_budget_over_a_group_of_each_tiled_width(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for pt in F.PLANE_TYPES:
        rows, refs = placed(clamp, pt), priced(oracle, mode, clamp, pt)
        for weighted, skip in F.FORMS4:
            for form in ((1, F.TILED), (4, F.TILED)):
                ids = F.entries_of_form(form, pt, weighted)  # every entry that runs in this form: ONE group, one budget
                name = (pt, form, weighted, skip)
                assert len(ids) >= 3 and assert_form(rows, ids, pt, weighted, want=form) == form
                ps, hws = [refs[i]["p"] for i in ids], [refs[i]["hw"] for i in ids]
                wts = [refs[i]["wt"] if weighted else refs[i]["ones"] for i in ids]
                f_plain = W.group_f(L, ps, wts) if weighted else V.group_f(L, ps)
                f = S.group_f(L, ps, wts, hws) if skip else f_plain
                budget = V.budget_of(*f_plain([0.0, 16.0]))
                want = V.search(f, budget)
                assert want["status"] == 0 and 0.0 < want["lam"] < 16.0, (name, want)
                got = gmc.quantize_to_budget_batch(*([rows[i][k] for i in ids] for k in range(4)), budget, groups=[0] * len(ids), per_channel=True,
                                                   **kwargs(rows, ids, weighted, skip))
                assert assert_form(rows, ids, pt, weighted, outs=[g.y for g in got]) == form
                assert sum(V.stream_bytes(L, g.bits_q_after) for g in got) == want["bytes_pred"] <= budget, name
                for i, g in zip(ids, got):
                    assert isinstance(g, BudgetQuantized)
                    assert np.float64(g.lam).tobytes() == np.float64(want["lam"]).tobytes(), (name, i, g.lam, want["lam"])  # bit for bit
                    assert (g.bytes_pred, g.passes, g.budget_met) == (want["bytes_pred"], want["passes"], True), (name, i, g, want)
                    check(g, ref_rdoq(oracle, mode, clamp, refs[i], want["lam"], weighted, skip), skip, (name, i))
                    q = gmc.quantize_rdo(*rows[i][:4], g.lam, per_channel=True, **kwargs(rows, [i], weighted, skip, batch=False))
                    assert qkey(g) == qkey(q), (name, i)


# ---- 5. batches -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,clamp", MODE_CLAMP)
def test_batches_of_unequal_items_equal_the_single_calls(mode, clamp):
    """the whole 1-wide tiled part of the corpus in ONE call - unequal M and hw, an item without channels in the middle - and the same
    with one 4-wide item appended, which changes nobody's form: every item's result is that of its single call, on every run"""
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for pt in F.PLANE_TYPES:
        rows = list(placed(clamp, pt))
        pdt = rows[0][1].dtype
        empty = (torch.zeros((1, 0, 3, 7), device=DEV), *(torch.zeros((1, 0, 3, 7), dtype=pdt, device=DEV) for _ in range(3)),
                 torch.zeros((0,), device=DEV), torch.ones((3, 7), device=DEV))
        rows.append(empty)
        for weighted, skip in F.FORMS4:
            ids = F.entries_of_form((1, F.TILED), pt, weighted)
            ids = ids[:len(ids) // 2] + [N] + ids[len(ids) // 2:]  # (N: the item with M = 0, hw = 21)
            four = [i for i in F.entries_of_form((4, F.TILED), pt, weighted) if F.ODD_CORPUS[i][1] * F.ODD_CORPUS[i][2] == 260][0]
            one_kw = lambda i: kwargs(rows, [i], weighted, skip, batch=False)  # noqa: E731
            singles_q = {i: gmc.quantize_rdo(*rows[i][:4], F.LAM, per_channel=True, **one_kw(i)) for i in ids + [four]}
            singles_c = {i: gmc.rd_curve(*rows[i][:4], LAMS16, **one_kw(i)) for i in ids + [four]}
            assert (singles_q[N].n_changed, singles_q[N].bits_q_after, singles_q[N].y.numel(), singles_c[N].n_symbols) == (0, 0, 0, 0)
            for sel in (ids, ids + [four]):
                name = (pt, weighted, skip, len(sel))
                assert_form(rows, sel, pt, weighted, want=(1, F.TILED))
                cols = [[rows[i][k] for i in sel] for k in range(4)]
                kw = kwargs(rows, sel, weighted, skip)
                qs = gmc.quantize_rdo_batch(*cols, F.LAM, per_channel=True, **kw)
                assert_form(rows, sel, pt, weighted, want=(1, F.TILED), outs=[q.y for q in qs])
                assert [qkey(q) for q in qs] == [qkey(singles_q[i]) for i in sel], name
                cs = gmc.rd_curve_batch(*cols, LAMS16, **kw)
                assert [ckey(c) for c in cs] == [ckey(singles_c[i]) for i in sel], name
                assert [qkey(q) for q in gmc.quantize_rdo_batch(*cols, F.LAM, per_channel=True, **kw)] == [qkey(q) for q in qs], name
                assert [ckey(c) for c in gmc.rd_curve_batch(*cols, LAMS16, **kw)] == [ckey(c) for c in cs], name
                if not weighted and not skip:
                    es = gmc.estimate_bits_batch(*cols, per_channel=True, per_latent=True)
                    assert [ekey(e) for e in es] == [ekey(gmc.estimate_bits(*rows[i][:4], per_channel=True, per_latent=True)) for i in sel], name
                    assert [ekey(e) for e in gmc.estimate_bits_batch(*cols, per_channel=True, per_latent=True)] == [ekey(e) for e in es], name


# ---- 6. logits ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", F.MODES)
def test_logits_in_the_1_wide_forms(oracle, mode):
    """one 1-wide tiled and one 1-wide linear entry with the weights given as logits: the plain call - and the reference - on the
    weights the kernels' own softmax over K (fgmm_softmax4_hip, rows (n, 4)) makes of them"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    rows = placed(True, "f32")
    for i, form in ((5, (1, F.TILED)), (10, (1, F.LIN))):
        M, h, w, _ = F.ODD_CORPUS[i]
        case = F.corpus_case(i, True)
        cw, pw = F.factors(i)
        lg = np.log(case[3]).astype(np.float32)
        lg_rows = dv(lg.reshape(4, M * h * w).T)
        pi_d = torch.empty_like(lg_rows)
        torch.cuda.synchronize()
        _lib.check(L.fgmm_softmax4_hip(ctx, None, lg_rows.data_ptr(), pi_d.data_ptr(), M * h * w))
        pi = np.ascontiguousarray(pi_d.cpu().numpy().T).reshape(1, 4 * M, h, w)
        y, s, m = rows[i][:3]
        r = dict(case=(case[0], case[1], case[2], pi), p=V.price(oracle, L, mode, case[0], case[1], case[2], pi), cw=cw, pw=pw, hw=h * w)
        for weighted, skip in F.FORMS4:
            name = (i, weighted, skip)
            kw = kwargs(rows, [i], weighted, skip, batch=False)
            t_lg, t_pi = (y, s, m, dv(lg)), (y, s, m, dv(pi))
            for t in (t_lg, t_pi):
                assert F.form_of_one(*t, pos_w=rows[i][5] if weighted else False) == form, name
            q = gmc.quantize_rdo(*t_lg, F.LAM, weights_are_logits=True, per_channel=True, **kw)
            assert qkey(q) == qkey(gmc.quantize_rdo(*t_pi, F.LAM, per_channel=True, **kw)), name
            check(q, ref_rdoq(oracle, mode, True, r, F.LAM, weighted, skip), skip, name)
            assert ckey(gmc.rd_curve(*t_lg, LAMS16, weights_are_logits=True, **kw)) == ckey(gmc.rd_curve(*t_pi, LAMS16, **kw)), name
        e = gmc.estimate_bits(y, s, m, dv(lg), weights_are_logits=True, per_channel=True, per_latent=True)
        assert ekey(e) == ekey(gmc.estimate_bits(y, s, m, dv(pi), per_channel=True, per_latent=True)), i
        assert e.bits_q == ref_rate(oracle, mode, True, r["case"])["bits_q"], i
