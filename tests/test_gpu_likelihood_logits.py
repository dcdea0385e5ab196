"""GPU (-m gpu): the likelihood from the parameter head's logits (include/flashgmm_amd.h section 3h; the LOGITS forms of like_kernel and
like_bwd_kernel in fgmm_like.hip, fgmm_like.cpp) - through the two C entry points, ``GaussianMixtureConditional.forward / rate_bits /
likelihood(..., weights_are_logits=True)``, ``forward_params / rate_bits_params`` and ``GaussianMixtureConditionalLatentCodec(...,
fuse_forward_softmax=True)``.

Two yardsticks, named per test:
  equivalence  the logits call equals, bit for bit, the plain call (section 3g) on the float32 planes P that fgmm_softmax4_hip makes of the
               logits - the map, v, bits_q, n_nonfinite, dy, dscales, dmeans - and its dweights equals Q.dlogits(P, the plain call's
               dweights), section 3h's three lines evaluated by torch on the GPU.  NaNs compare as NaNs, everything else by its bits.
  accuracy     E_k <= 2 * E_ref + 2^-23 against float64, the rule of tests/test_gpu_likelihood.py, E_ref torch's float32 evaluation on
               the GPU (torch.softmax, R.forward, R.backward, Q.dlogits).  For the logits' gradient the error is measured against
               Q.mag, the terms dl_k is a difference of, not against |x64|: where pi -> 1 the difference dpi_k - t cancels and the last
               bits of pi decide (a CPU stand-in of the kernel fails the rule against |x64| in region (a), 7.6e-2 against 1.3e-2, and
               meets it against mag in every region).  Every figure is printed before it is asserted (run with -s).
Every case of the instantiation test asserts its launch form on the addresses it really passes (R.launch_form) before the call."""
import itertools

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec
from test_gpu_likelihood import DEV, LB32, _fill, check_accuracy, dv, make
from test_gpu_likelihood_edges import DT, GB, all_same, assert_form, fitem, off, same
from test_gpu_streams import delay, pending, snapshot, streams  # noqa: F401  (the stream case runs in that module's manner, on its helpers)
from test_likelihood_logits_cpu import INSTANTIATION_CASES
from tests import like_logits_ref as Q
from tests import like_ref as R

pytestmark = pytest.mark.gpu

LOGITS = _lib.FGMM_PARAMS_LOGITS
F32 = torch.float32


@pytest.fixture(scope="module")
def gmc():
    return GaussianMixtureConditional(K=4).eval()


def same_n(a, b):
    """NaN where the other is NaN, bit for bit elsewhere (0 differs from -0)"""
    if a is None or b is None:
        return a is None and b is None
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and torch.equal(na, nb) and torch.equal(a[~na].view(torch.int32), b[~nb].view(torch.int32))


def make_l(seed, B, M, h, w, dtype=F32):
    """``make`` with the weights replaced by logits, 2 * N(0, 1) -> y, scales, means, logits, g on the GPU"""
    y, s, m, _, g = make(seed, B, M, h, w, dtype=dtype)
    lg = dv((2.0 * np.random.default_rng(seed + 1).standard_normal((B, 4 * M, h, w))).astype(np.float32)).to(dtype)
    return [y, s, m, lg, g]


def one_l(seed, M, h, w, dt):
    t = make_l(seed, 1, M, h, w, dtype=DT[dt])
    return tuple(x[0] for x in t[:4]), t[4][0]


def softmax4_planes(lg):
    """[4M, h, w] logits (widened exactly) -> the float32 planes of the weights fgmm_softmax4_hip makes of them, rows (n, 4)"""
    rows = lg.to(F32).reshape(4, -1).t().contiguous()
    out = torch.empty_like(rows)
    if rows.size(0):
        torch.cuda.current_stream().synchronize()
        _lib.check(_lib.lib().fgmm_softmax4_hip(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, rows.data_ptr(), out.data_ptr(), rows.size(0)))
    return out.t().contiguous().reshape(lg.shape)


def plain_of(item):
    """the plain call's item: fresh, dense, aligned float32 tensors, the weights fgmm_softmax4_hip's"""
    y, s, m, lg = item
    return (y.clone(), s.to(F32).clone(), m.to(F32).clone(), softmax4_planes(lg))


def _flags(flags, logits, i):
    if flags is None:
        return LOGITS if logits else 0
    return flags[i] if isinstance(flags, (list, tuple)) else flags


def _new(like, fill, shape=None):
    shape = like.shape if shape is None else shape
    return torch.empty(shape, dtype=F32, device=DEV) if fill is None else torch.full(shape, fill, dtype=F32, device=DEV)


def _ptr(t):
    return None if t is None else t.data_ptr()


def raw_fwd(items, rnd, logits=True, sb=R.SB, lb=R.LB, K=4, flags=None, fill=None, outs=None, sizes=None):
    """fgmm_gmc_likelihood_logits_batch (``logits``) or fgmm_gmc_likelihood_batch on items (y [M, h, w], scales, means, weights [4M, h, w])
    on the current stream -> (rc, [(like, v, bits_q, n_nonfinite)]); ``outs``: per item the caller's (like, v), None for NULL"""
    arr = (_lib.fgmm_like_item * len(items))()
    res = []
    for i, (it, (y, s, m, w)) in enumerate(zip(arr, items)):
        _fill(it, y, s, m, w, K, _flags(flags, logits, i), sizes[i] if sizes else None)
        like, v = outs[i] if outs is not None else (_new(y, fill), _new(y, fill))
        it.like_out, it.v_out = _ptr(like), _ptr(v)
        res.append((like, v))
    if fill is not None:
        torch.cuda.current_stream().synchronize()
    call = _lib.lib().fgmm_gmc_likelihood_logits_batch if logits else _lib.lib().fgmm_gmc_likelihood_batch
    rc = call(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, arr, len(items), int(rnd), sb, lb)
    return rc, [(like, v, int(it.bits_q), int(it.n_nonfinite)) for it, (like, v) in zip(arr, res)]


def raw_bwd(items, gs, rnd, g_bits=None, logits=True, sb=R.SB, lb=R.LB, K=4, flags=None, fill=None, outs=None, sizes=None):
    """the backward entry point of the same section -> (rc, [[dy, dscales, dmeans, dweights]]); gs: the items' g_like, or None with g_bits"""
    arr = (_lib.fgmm_like_grad_item * len(items))()
    res = []
    for i, (it, (y, s, m, w)) in enumerate(zip(arr, items)):
        _fill(it, y, s, m, w, K, _flags(flags, logits, i), sizes[i] if sizes else None)
        o = outs[i] if outs is not None else [_new(y, fill)] + [_new(s, fill) for _ in range(3)]
        it.dy, it.dscales, it.dmeans, it.dweights = (_ptr(t) for t in o)
        if gs is not None:
            it.g_like = gs[i].data_ptr()
        else:
            it.g_bits = g_bits[i]
        res.append(o)
    if fill is not None:
        torch.cuda.current_stream().synchronize()
    call = _lib.lib().fgmm_gmc_likelihood_logits_backward_batch if logits else _lib.lib().fgmm_gmc_likelihood_backward_batch
    rc = call(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, arr, len(items), int(rnd), sb, lb)
    return rc, res


def dl_of(P, dw):
    """section 3h's three lines by torch on the GPU, on one item's planes"""
    return Q.dlogits(P.unsqueeze(0), dw.unsqueeze(0))[0]


def check_equiv(items, gs, rnd, sb=R.SB, lb=R.LB, sizes=None, what=None, fouts=None, bouts=None):
    """equivalence of one batch: the logits calls on ``items`` against the plain calls on P.  An item of ``sizes`` with M = 0 or hw = 0
    gets nothing written and nothing counted.  ``fouts`` / ``bouts``: the caller's outputs of the logits calls, per item (like, v) and
    [dy, dscales, dmeans, dweights]"""
    n = len(items)
    for t in [t for o in (fouts or []) + (bouts or []) for t in o]:
        t.fill_(-7.0)
    live = [i for i in range(n) if sizes is None or sizes[i][0] * sizes[i][1] > 0]
    plain = [plain_of(items[i]) for i in live]
    (rc, f), (rc2, pf) = raw_fwd(items, rnd, sb=sb, lb=lb, fill=-7.0, outs=fouts, sizes=sizes), raw_fwd(plain, rnd, logits=False, sb=sb, lb=lb)
    assert rc == 0 and rc2 == 0, what
    for j, i in enumerate(live):
        assert same_n(f[i][0], pf[j][0]) and same_n(f[i][1], pf[j][1]) and f[i][2:] == pf[j][2:], (what, i, rnd, "forward")
    for i in set(range(n)) - set(live):
        assert f[i][2:] == (0, 0) and torch.all(f[i][0] == -7.0) and torch.all(f[i][1] == -7.0), (what, i)
    rc, r = raw_fwd(items, rnd, sb=sb, lb=lb, outs=[(None, None)] * n, sizes=sizes)  # the rate alone
    assert rc == 0 and [x[2:] for x in r] == [x[2:] for x in f], what
    gbs = list(GB[:n]) if n <= len(GB) else [GB[i % len(GB)] for i in range(n)]
    for g_like, g_bits in ((gs, None), (None, gbs)):
        for t in [t for o in bouts or [] for t in o]:
            t.fill_(-7.0)
        rc, o = raw_bwd(items, g_like, rnd, g_bits=g_bits, sb=sb, lb=lb, fill=-7.0, outs=bouts, sizes=sizes)
        rc2, po = raw_bwd(plain, None if g_like is None else [g_like[i].clone() for i in live], rnd, g_bits=None if g_bits is None else [g_bits[i] for i in live],
                          logits=False, sb=sb, lb=lb)
        assert rc == 0 and rc2 == 0, what
        for j, i in enumerate(live):
            for name, a, b in zip(R.GRADS[:3], o[i], po[j]):
                assert same_n(a, b), (what, i, rnd, name, g_bits)
            assert same_n(o[i][3], dl_of(plain[j][3], po[j][3])), (what, i, rnd, "dlogits", g_bits)
        for i in set(range(n)) - set(live):
            assert all(torch.all(t == -7.0) for t in o[i]), (what, i)
    return f, plain


# ---- 1. equivalence on the logits corpus and on planted non-finite logits ----------------------------------------------------------------
@pytest.mark.parametrize("sb,lb", [(R.SB, R.LB), R.BOUNDS[0]])
@pytest.mark.parametrize("data", ["corpus", "nonfinite"])
def test_logits_call_equals_the_plain_call_on_the_kernels_own_weights(data, sb, lb):
    """equivalence, with round 0 and 1, through g_like and through g_bits, at the default bounds and without a likelihood bound"""
    arrays = Q.logits_corpus() if data == "corpus" else Q.nonfinite_logits()
    y, s, m, lg, g = (dv(a)[0] for a in arrays[:5])
    for rnd in (False, True):
        f, plain = check_equiv([(y, s, m, lg)], [g], rnd, sb, lb, what=data)
        if data == "nonfinite":
            P, like = plain[0][3].reshape(4, -1), f[0][0].reshape(-1)
            rows = Q.logit_rows(arrays[3])
            for kind, i, k in arrays[5]:
                if kind == "nan":  # weight 0 for the NaN logit, the others a softmax of three
                    others = [j for j in range(4) if j != k]
                    assert float(P[k, i]) == 0.0 and bool(torch.isfinite(P[:, i]).all()) and abs(float(P[:, i].sum()) - 1) < 1e-6
                    e = np.exp(rows[i, others].astype(np.float64) - rows[i, others].max())
                    assert np.allclose(P[others, i].cpu().numpy(), e / e.sum(), rtol=0, atol=1e-6)
                elif kind == "ninf":
                    assert float(P[k, i]) == 0.0 and abs(float(P[:, i].sum()) - 1) < 1e-6
                else:  # a +inf, or four -inf: NaN weights, a NaN likelihood, left out of the sum and counted
                    assert bool(torch.isnan(P[:, i]).all()) and bool(torch.isnan(like[i]))
            assert f[0][3] == 8 if lb > 0 else f[0][3] >= 8 + 256  # (no bound: region (c)'s exact zeros are left out too)


# ---- 2. every instantiation of the logits form ---------------------------------------------------------------------------------------------
SHAPES = {"old_corpus": [(8, 16, 16)], "old_hw255": [(4, 15, 17)], "old_B3_hw64": [(2, 8, 8)] * 3, "old_offset_hw256": [(8, 16, 16)], "old_hw256": [(4, 16, 16)],
          "old_hw264": [(4, 12, 22)], "old_hw252": [(4, 14, 18)], "old_hw512": [(2, 16, 32)] * 2, "a_hw35": [(3, 5, 7)], "a_planes_off": [(3, 8, 8)] * 2,
          "b_unequal": [(2, 16, 16), (5, 16, 16), (1, 16, 32)], "b_M0": [(2, 16, 16)] * 2, "b_hw0": [(2, 16, 16)] * 2, "c_chunk_hw64": [(3, 8, 8)] * 2,
          "c_chunk_hw35": [(3, 5, 7)] * 2}


def case_items(case, dt):
    """-> (items, gs, sizes) of a case of R.CASES, laid out as the case says"""
    items, gs = map(list, zip(*(one_l(6100 + 10 * len(case) + i, *shp, dt) for i, shp in enumerate(SHAPES[case]))))
    sizes = None
    if case == "old_offset_hw256":
        items = [tuple(off(t, 4) for t in it) for it in items]
        gs = [off(g, 4) for g in gs]
    elif case == "a_planes_off":
        items = [(it[0],) + tuple(off(t, 2) for t in it[1:]) for it in items]
    elif case in ("b_M0", "b_hw0"):
        sizes = [(0, 256) if case == "b_M0" else (2, 0), (2, 256)]
    elif case.startswith("c_chunk"):  # the chunk views of a [2, 12M, h, w] tensor: what a parameter network's output gives
        M, h, w = SHAPES[case][0]
        views = items[0][1].new_empty((2, 12 * M, h, w)).chunk(3, 1)
        for i, it in enumerate(items):
            for v, t in zip(views, it[1:]):
                v[i].copy_(t)
        assert not any(v.is_contiguous() for v in views)
        items = [(it[0],) + tuple(v[i] for v in views) for i, it in enumerate(items)]
    return items, gs, sizes


@pytest.mark.parametrize("case,dt", INSTANTIATION_CASES)
def test_every_instantiation_of_the_logits_form(case, dt):
    """equivalence, on the launch forms of R.CASES - asserted for the forward and the backward call on the addresses really passed.
    tests/test_likelihood_logits_cpu.py proves the union of the chosen cases' forms is all 28 instantiations."""
    items, gs, sizes = case_items(case, dt)
    n = len(items)
    size = lambda i: sizes[i] if sizes else None  # noqa: E731
    fouts = [(_new(it[0], None), _new(it[0], None)) for it in items]
    bouts = [[_new(it[0], None)] + [_new(it[1], None) for _ in range(3)] for it in items]
    assert all(t.data_ptr() % 16 == 0 for o in fouts + bouts for t in o)
    assert_form(case, dt, [fitem(*items[i], rest=fouts[i], size=size(i)) for i in range(n)], False)
    assert_form(case, dt, [fitem(*items[i], rest=[gs[i]] + bouts[i], size=size(i)) for i in range(n)], True)
    for rnd in (True, False):
        check_equiv(items, gs, rnd, sizes=sizes, what=(case, dt), fouts=fouts, bouts=bouts)


# ---- 3. two-byte logits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (1, 4, 16, 16), (2, 2, 16, 32)])  # 1, 4 and 8 positions per lane (backward: 1, 4, 4)
def test_two_byte_logits_equal_float32_planes_holding_the_widened_values(dt, shape):
    y, s, m, lg, g = make_l(6300 + shape[2], *shape, dtype=DT[dt])
    assert lg.dtype == DT[dt]
    B = shape[0]
    items2 = [(y[i], s[i], m[i], lg[i]) for i in range(B)]
    items4 = [(y[i], s[i].to(F32), m[i].to(F32), lg[i].to(F32)) for i in range(B)]
    vec = {35: 1, 256: 4, 512: 8}[shape[2] * shape[3]]
    assert R.launch_form([fitem(*it) for it in items2], True, False)[0] == vec and R.launch_form([fitem(*it) for it in items4], False, False)[0] == min(vec, 4)
    for rnd in (True, False):
        (rc2, f2), (rc4, f4) = raw_fwd(items2, rnd), raw_fwd(items4, rnd)
        assert rc2 == 0 and rc4 == 0
        for a, b in zip(f2, f4):
            assert same(a[0], b[0]) and same(a[1], b[1]) and a[2:] == b[2:] and a[3] == 0
        for gs, gb in ((list(g), None), (None, list(GB[:B]))):
            (rc2, o2), (rc4, o4) = raw_bwd(items2, gs, rnd, g_bits=gb), raw_bwd(items4, gs, rnd, g_bits=gb)
            assert rc2 == 0 and rc4 == 0 and all(all_same(a, b) for a, b in zip(o2, o4)), (rnd, gb)


# ---- 4. accuracy against float64, per region of the logits corpus ---------------------------------------------------------------------------
def check_acc(what, got, ref32, x64, D, mask, floor):
    """E = max |x - x64| / max(D, floor) on the rows of ``mask``: E_k <= 2 * E_ref + 2^-23, both printed first"""
    e = lambda x: float((np.abs(x.astype(np.float64) - x64) / np.maximum(D, floor))[mask].max())  # noqa: E731
    e_ref, e_k = e(ref32), e(got)
    print(f"accuracy {what:28s} E_ref {e_ref:.3e}  E_k {e_k:.3e}  ratio {e_k / e_ref if e_ref else float('inf') if e_k else 1.0:.3f}")
    assert e_k <= 2.0 * e_ref + 2.0 ** -23, (what, e_ref, e_k)


@pytest.fixture(scope="module")
def corpus_ref():
    """computed once, left unchanged: the logits corpus, its float64 values and torch's float32 evaluation on the GPU"""
    cpu = [torch.from_numpy(a) for a in Q.logits_corpus()]
    gpu = [t.to(DEV) for t in cpu]
    pi64, pi32 = Q.softmax_planes(cpu[3]), Q.softmax_planes(gpu[3], F32)
    out = dict(cpu=cpu, gpu=gpu)
    for rnd in (False, True):
        f64, f32 = R.forward(*cpu[:3], pi64, rnd=rnd, dtype=torch.float64), R.forward(*gpu[:3], pi32, rnd=rnd)
        dpi64 = R.backward(f64, cpu[4])["dweights"]
        out[rnd] = dict(like64=f64["out"].numpy(), L64=f64["L"].numpy(), like32=f32["out"].cpu().numpy(),
                        dl64=Q.reference_gradients_logits(*cpu, rnd=rnd)[1]["dweights"].numpy(), mag=Q.mag(pi64, dpi64).numpy(),
                        dl32=Q.dlogits(pi32, R.backward(f32, gpu[4])["dweights"]).cpu().numpy())
    return out


@pytest.mark.parametrize("rnd", [False, True])
def test_accuracy_against_float64_per_region(corpus_ref, rnd):
    """accuracy: the map against |x64| with the likelihood bound as the floor; the logits' gradient against Q.mag with 1e-6 of the region's
    largest |x64| as the floor, the rows whose float64 L lies within 1e-3 of the bound left out (tests/test_likelihood_logits_cpu.py:
    none of 2048)."""
    y, s, m, lg, g = (t[0] for t in corpus_ref["gpu"])
    ref = corpus_ref[rnd]
    (rc, [f]), (rc2, [o]) = raw_fwd([(y, s, m, lg)], rnd), raw_bwd([(y, s, m, lg)], [g], rnd)
    assert rc == 0 and rc2 == 0
    like, dl = f[0].cpu().numpy()[None], o[3].cpu().numpy()[None]
    keep = ~R.near_bound(ref["L64"])
    assert keep.mean() >= 0.99
    for name in R.REGIONS:
        check_acc(f"likelihood rnd={int(rnd)} ({name})", like, ref["like32"], ref["like64"], np.abs(ref["like64"]), R.region_mask(name) & keep, LB32)
    rows = np.tile(keep, (1, 4, 1, 1))
    for name in R.REGIONS:
        mask = R.plane_mask(name) & rows
        floor = max(1e-6 * float(np.abs(ref["dl64"][mask]).max()), 1e-300)
        check_acc(f"dlogits rnd={int(rnd)} ({name})", dl, ref["dl32"], ref["dl64"], ref["mag"], mask, floor)


# ---- 5. the public interface ------------------------------------------------------------------------------------------------------------------
def leaves_of(*ts):
    return [t.detach().requires_grad_(True) for t in ts]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_weights_are_logits_through_autograd_equals_the_raw_calls(gmc, dt):
    """equivalence of layers: forward / likelihood / rate_bits with weights_are_logits=True give the raw calls' outputs, and autograd
    their gradients (rounded once to the planes' dtype)"""
    y, s, m, lg, g = make_l(6500, 2, 3, 8, 8, dtype=DT[dt])
    items = [(y[i], s[i], m[i], lg[i]) for i in range(2)]
    for rnd in (True, False):
        lv = leaves_of(y, s, m, lg)
        v, like = gmc.likelihood(*lv, round=rnd, weights_are_logits=True)
        like.backward(g)
        (rc, f), (rc2, o) = raw_fwd(items, rnd), raw_bwd(items, list(g), rnd)
        assert rc == 0 and rc2 == 0
        assert same(like.detach(), torch.stack([x[0] for x in f])) and torch.equal(v.detach(), torch.stack([x[1] for x in f]) if rnd else y)
        assert (lv[0].grad is None) == rnd and (rnd or same(lv[0].grad, torch.stack([x[0] for x in o])))
        for j in (1, 2, 3):
            assert lv[j].grad.dtype == DT[dt] and same(lv[j].grad, torch.stack([x[j] for x in o]).to(DT[dt])), (rnd, j)
    out, like2 = gmc(y, s, m, lg, weights_are_logits=True)  # evaluation mode: the rounded call
    assert rc == 0 and torch.equal(out, torch.round(y)) and same(like2, gmc.likelihood(y, s, m, lg, round=True, weights_are_logits=True)[1])
    lv = leaves_of(y, s, m, lg)
    outputs, bits, nf = gmc.rate_bits(*lv, return_nonfinite=True, weights_are_logits=True)
    (bits * torch.tensor(GB[:2], dtype=torch.float64, device=DEV)).sum().backward()
    (rc, f), (rc2, o) = raw_fwd(items, True), raw_bwd(items, None, True, g_bits=list(GB[:2]))
    assert rc == 0 and rc2 == 0 and bits.tolist() == [x[2] * 2.0 ** -32 for x in f] and nf.tolist() == [0, 0] and torch.equal(outputs, torch.round(y))
    assert lv[0].grad is None and all(same(lv[j].grad, torch.stack([x[j] for x in o]).to(DT[dt])) for j in (1, 2, 3))
    with pytest.raises(RuntimeError):  # K = 4 only, as everywhere
        GaussianMixtureConditional(K=3).likelihood(y, s[:, :9], m[:, :9], lg[:, :9], weights_are_logits=True)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hw", [(8, 8), (5, 7), (16, 32)])
def test_forward_params_is_forward_on_the_chunks(gmc, dt, hw):
    """equivalence of layers: outputs and every gradient of forward_params / rate_bits_params equal those of
    forward / rate_bits(y, *params.chunk(3, 1), weights_are_logits=True) bit for bit; params.grad is ONE contiguous tensor of params'
    shape and dtype; y gets no gradient in evaluation mode; in training mode the noised output is priced"""
    M, (h, w) = 3, hw
    y, s, m, lg, g = make_l(6600 + h, 2, M, h, w, dtype=DT[dt])
    params = torch.cat([s, m, lg], 1)
    for training in (False, True):
        a_y, a_p = leaves_of(y, params)
        torch.manual_seed(41)
        out_a, like_a = gmc.forward_params(a_y, a_p, training=training)
        like_a.backward(g)
        b_y, b_p = leaves_of(y, params)
        torch.manual_seed(41)
        out_b, like_b = gmc(b_y, *b_p.chunk(3, 1), training=training, weights_are_logits=True)
        like_b.backward(g)
        assert torch.equal(out_a, out_b) and same(like_a.detach(), like_b.detach())
        assert a_p.grad.is_contiguous() and a_p.grad.shape == params.shape and a_p.grad.dtype == params.dtype and same(a_p.grad, b_p.grad)
        if training:
            d = out_a.detach().double() - y.double()
            assert float(d.min()) >= -0.5 and float(d.max()) <= 0.5 and float(d.std()) > 0.2
            assert same(like_a.detach(), gmc.likelihood(out_a.detach(), *params.chunk(3, 1), weights_are_logits=True)[1])  # the noised values are priced
            assert same(a_y.grad, b_y.grad) and bool(a_y.grad.any())
        else:
            assert torch.equal(out_a, torch.round(y)) and a_y.grad is None and b_y.grad is None
        # the rate
        a_y, a_p = leaves_of(y, params)
        torch.manual_seed(43)
        out_a, bits_a, nf_a = gmc.rate_bits_params(a_y, a_p, training=training, return_nonfinite=True)
        (bits_a * torch.tensor(GB[:2], dtype=torch.float64, device=DEV)).sum().backward()
        b_y, b_p = leaves_of(y, params)
        torch.manual_seed(43)
        out_b, bits_b = gmc.rate_bits(b_y, *b_p.chunk(3, 1), training=training, weights_are_logits=True)
        (bits_b * torch.tensor(GB[:2], dtype=torch.float64, device=DEV)).sum().backward()
        assert torch.equal(out_a, out_b) and torch.equal(bits_a, bits_b) and bits_a.dtype == torch.float64 and nf_a.tolist() == [0, 0]
        assert a_p.grad.is_contiguous() and a_p.grad.dtype == params.dtype and same(a_p.grad, b_p.grad) and (a_y.grad is None) == (not training)
        assert training is False or same(a_y.grad, b_y.grad)
    # only the latent asks for a gradient: no planes are written, dy is the full call's
    b_y = y.detach().requires_grad_(True)
    torch.manual_seed(1)
    out, like = gmc.forward_params(b_y, params, training=True)
    like.backward(g)
    ref_y = out.detach().requires_grad_(True)
    gmc.likelihood(ref_y, *params.chunk(3, 1), weights_are_logits=True)[1].backward(g)
    assert same(b_y.grad, ref_y.grad) and bool(b_y.grad.any())
    with pytest.raises(RuntimeError):
        gmc.forward_params(y, params[:, :-1])


class Affine(torch.nn.Module):
    """a parameter network of two element-wise operations"""

    def __init__(self, C):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.full((1, C, 1, 1), 1.0625))
        self.bias = torch.nn.Parameter(torch.full((1, C, 1, 1), 0.03125))

    def forward(self, x):
        return x * self.scale + self.bias


def test_latent_codec_with_fuse_forward_softmax():
    """equivalence of layers: the codec's forward with the option is forward_params of its own parameter network's output.  accuracy: against
    the same codec with the option off - torch.softmax then the plain kernel - the likelihoods agree by the rule of the accuracy test,
    the un-fused forward in torch's place"""
    M, h, w = 6, 8, 12
    rng = np.random.default_rng(6700)
    y = dv((rng.standard_normal((2, M, h, w)) * 3).astype(np.float32))
    ctx = rng.standard_normal((2, 12 * M, h, w)).astype(np.float32)
    ctx[:, :4 * M] = np.exp(ctx[:, :4 * M])  # scales
    ctx[:, 8 * M:] *= 2.0
    ctx = dv(ctx)
    net = Affine(12 * M).to(DEV)
    fused = GaussianMixtureConditionalLatentCodec(K=4, entropy_parameters=net, fuse_forward_softmax=True).to(DEV)
    plain = GaussianMixtureConditionalLatentCodec(K=4, entropy_parameters=net).to(DEV)
    gmc = fused.gaussian_mixture_conditional
    for training in (False, True):
        fused.train(training), plain.train(training)
        torch.manual_seed(77)
        out = fused(y, ctx)
        torch.manual_seed(77)
        y_hat, like = gmc.forward_params(y, net(ctx), training=training)
        assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y"}
        assert torch.equal(out["y_hat"], y_hat) and same(out["likelihoods"]["y"].detach(), like.detach())
        torch.manual_seed(77)
        ref = plain(y, ctx)
        assert torch.equal(ref["y_hat"], out["y_hat"])
        p64 = net(ctx).detach().double().cpu()
        f64 = R.forward(out["y_hat"].detach().double().cpu(), p64[:, :4 * M], p64[:, 4 * M:8 * M], Q.softmax_planes(p64[:, 8 * M:]), rnd=False, dtype=torch.float64)
        check_accuracy(f"codec training={int(training)}", out["likelihoods"]["y"].detach().cpu().numpy(), ref["likelihoods"]["y"].detach().cpu().numpy(),
                       f64["out"].numpy(), floor=LB32)
    # the rate term of a training loss reaches the parameter network and the codec's input
    fused.train()
    ctx_leaf = ctx.detach().requires_grad_(True)
    (-torch.log2(fused(y, ctx_leaf)["likelihoods"]["y"])).sum().backward()
    assert ctx_leaf.grad is not None and torch.isfinite(ctx_leaf.grad).all() and ctx_leaf.grad.abs().sum() > 0
    assert net.scale.grad is not None and torch.isfinite(net.scale.grad).all() and net.scale.grad.abs().sum() > 0


# ---- 6. partial outputs and refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["d_hw256", "d_hw35"])
def test_every_subset_of_the_four_outputs(case):
    """equivalence of layouts, at 4 positions per lane on the linear grid and at 1 on the tiled one: the outputs that are asked for equal
    the full call's, the memory of those that are not stays as it was.  The four outputs are consecutive parts of one buffer, so a
    store through a wrong base would land in a part that is watched."""
    item, g = one_l(6800, 2, *{"d_hw256": (16, 16), "d_hw35": (5, 7)}[case], "f32")
    n = item[0].numel()
    counts = [n, 4 * n, 4 * n, 4 * n]
    bounds = np.cumsum([0] + counts)
    for gs, gb in (([g], None), (None, [GB[0]])):
        rc, [full] = raw_bwd([item], gs, False, g_bits=gb)
        assert rc == 0
        for subset in itertools.chain.from_iterable(itertools.combinations(range(4), k) for k in range(1, 5)):
            buf = torch.full((int(bounds[-1]),), -7.0, dtype=F32, device=DEV)
            parts = [buf[bounds[i]:bounds[i + 1]].view(full[i].shape) for i in range(4)]
            if subset == (0, 1, 2, 3):
                assert_form(case, "f32", [fitem(*item, rest=[g] + parts)], True)
            torch.cuda.current_stream().synchronize()
            rc, [o] = raw_bwd([item], gs, False, g_bits=gb, outs=[[parts[i] if i in subset else None for i in range(4)]])
            assert rc == 0, (subset, gb)
            for i in range(4):
                assert same(parts[i], full[i]) if i in subset else bool(torch.all(parts[i] == -7.0)), (subset, i, gb)


def test_refusals_write_nothing():
    """the new entry points refuse - FGMM_ERR_INVALID, nothing written - flags 0, a batch that mixes the forms, K = 3, section 3g's bound
    refusals, and a backward item whose outputs are all NULL"""
    y, s, m, lg, g = make_l(6900, 2, 4, 8, 8)
    items = [(y[i], s[i], m[i], lg[i]) for i in range(2)]
    bad = (dict(flags=0), dict(flags=[LOGITS, 0]), dict(flags=[0, LOGITS]), dict(flags=LOGITS | 2), dict(K=3), dict(sb=0.0), dict(sb=-1.0), dict(sb=float("inf")),
           dict(lb=-1e-9), dict(lb=float("nan")), dict(lb=float("inf")))
    for kw in bad:
        rc, f = raw_fwd(items, True, fill=-7.0, **kw)
        torch.cuda.synchronize()
        assert rc == 1 and all(torch.all(like == -7.0) and torch.all(v == -7.0) for like, v, _, _ in f), kw
        for gs, gb in ((list(g), None), (None, [1.5, 1.5])):
            rc, o = raw_bwd(items, gs, False, g_bits=gb, fill=-7.0, **kw)
            torch.cuda.synchronize()
            assert rc == 1 and all(torch.all(t == -7.0) for it in o for t in it), kw
    rc, o = raw_bwd(items, None, False, g_bits=[1.5, float("inf")], fill=-7.0)
    torch.cuda.synchronize()
    assert rc == 1 and all(torch.all(t == -7.0) for it in o for t in it)
    full = [torch.full_like(y[1], -7.0)] + [torch.full_like(s[1], -7.0) for _ in range(3)]
    rc, _ = raw_bwd(items, list(g), False, outs=[full, [None] * 4])  # the second item: every output NULL
    torch.cuda.synchronize()
    assert rc == 1 and all(torch.all(t == -7.0) for t in full)
    assert raw_fwd(items, True)[0] == 0  # (the same items are taken as they are)
    # the two entry points of section 3g keep refusing the flag
    assert raw_fwd(items, True, logits=False, flags=LOGITS)[0] == 1 and raw_bwd(items, list(g), False, logits=False, flags=LOGITS)[0] == 1


# ---- 7. the caller's-stream contract ----------------------------------------------------------------------------------------------------------
def test_logits_forward_and_backward_with_a_pending_producer(streams, delay):  # noqa: F811
    s1, s2, third = streams
    true, decoy = make_l(7000, 2, 4, 16, 16), make_l(7001, 2, 4, 16, 16)
    split = lambda t: [tuple(x[i] for x in t[:4]) for i in range(2)]  # noqa: E731
    (rc1, f_w), (rc2, o_w) = raw_fwd(split(true), False), raw_bwd(split(true), list(true[4]), False)
    assert rc1 == 0 and rc2 == 0 and not torch.equal(f_w[0][0], raw_fwd(split(decoy), False)[1][0][0])
    with pending(s1, delay, true, decoy) as t:
        rc, f = raw_fwd(split(t), False)
        f_3 = snapshot(third, [x[0] for x in f])
    assert rc == 0 and all(same(a, b[0]) for a, b in zip(f_3, f_w)) and [x[2:] for x in f] == [x[2:] for x in f_w]
    with pending(s2, delay, true, decoy) as t:
        rc, o = raw_bwd(split(t), list(t[4]), False)
        o_3 = snapshot(third, [x for it in o for x in it])
    assert rc == 0 and all_same(o_3, [x for it in o_w for x in it])
