"""GPU: the entropy bottleneck's forward() (include/flashgmm_amd.h section 3j) - ``fgmm_eb_likelihood`` /
``fgmm_eb_likelihood_backward`` through ctypes, and ``EntropyBottleneck`` / ``HyperLatentCodec.forward`` over them.

Accuracy goes by the project's rule (tests/test_gpu_likelihood.py): per region and quantity E = max |x32 - x64| / max(|x64|, floor) against
float64 - the fixture's values from the reference's own class on the corpus, elsewhere the float64 restatement of tests/eb_ref.py, which
tests/test_entropy_bottleneck_cpu.py ties to that class - once for torch float32 of the MIRRORED form on the GPU (E_ref; autograd through it
for gradients) and once for the kernels (E_k), and E_k <= 2 * E_ref + 2^-23 is required.  The floor is the likelihood bound for
likelihoods, 1e-6 times the quantity's largest float64 magnitude for a gradient.  Every figure is printed before it is asserted (-s).  A
kernel of the reference's written form fails the right tail: its error there is above 1 (test_entropy_bottleneck_cpu.py)."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest
import torch

from flashgmm_amd import EntropyBottleneck, _lib
from flashgmm_amd.latent_codecs import HyperLatentCodec
from test_gpu_streams import delay, pending, snapshot, streams  # noqa: F401  (the stream case runs in that module's manner, on its helpers)
from tests import eb_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB32 = R.f32(R.LB)
S = _lib.FGMM_EB_SLICE
GUARD = 4  # float32 elements either side of an output (16 bytes: the output keeps the alignment of its allocation)
GUARDVAL = -777.25


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def err(x, x64, floor, mask=None):
    e = np.abs(np.asarray(x, np.float64) - x64) / np.maximum(np.abs(x64), floor)
    return float(e[mask].max()) if mask is not None else float(e.max())


def check_accuracy(what, got, ref32, x64, mask=None, floor=None):
    """E_k <= 2 * E_ref + 2^-23 on the elements of `mask` (the module's docstring); floor None: a gradient's, from the quantity itself"""
    got, ref32, x64 = (np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t) for t in (got, ref32, x64))
    x64 = x64.reshape(got.shape)
    if floor is None:
        floor = max(1e-6 * float(np.abs(x64[mask] if mask is not None else x64).max()), 1e-300)
    e_ref, e_k = err(ref32.reshape(got.shape), x64, floor, mask), err(got, x64, floor, mask)
    print(f"accuracy {what:34s} E_ref {e_ref:.3e}  E_k {e_k:.3e}  ratio {e_k / e_ref if e_ref else float('inf') if e_k else 1.0:.3f}")
    assert e_k <= 2.0 * e_ref + 2.0 ** -23, (what, e_ref, e_k)


class Guarded:
    """a float32 device buffer of n elements pre-filled with NaN, between guard elements"""

    def __init__(self, n):
        self.n, self.raw = n, torch.full((n + 2 * GUARD,), GUARDVAL, dtype=torch.float32, device=DEV)
        self.t = self.raw[GUARD:GUARD + n]
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.raw[:GUARD] == GUARDVAL).all() and (self.raw[GUARD + self.n:] == GUARDVAL).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def raw_forward(x, theta, med, mode, lb=R.LB, like=True, v=True, host=True, stream=None):
    """fgmm_eb_likelihood on x [B, C, hw] -> (rc, like, v, bits_q, n_nonfinite, guards); a False output is passed as NULL"""
    B, Cn, hw = x.shape
    gl, gv = (Guarded(x.numel()) if want else None for want in (like, v))
    bits, nonf = np.full(B, -5, np.int64), np.full(B, -5, np.int64)
    call = _lib.fgmm_eb_call(x.data_ptr(), theta.data_ptr(), med.data_ptr(), B, Cn, hw, gl.t.data_ptr() if gl else None, gv.t.data_ptr() if gv else None,
                             bits.ctypes.data if host else None, nonf.ctypes.data if host else None, 0, 0)
    torch.cuda.current_stream().synchronize()
    rc = _lib.lib().fgmm_eb_likelihood(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, C.byref(call), mode, lb)
    shaped = lambda g: g.t.reshape(x.shape) if g else None  # noqa: E731
    return rc, shaped(gl), shaped(gv), bits, nonf, [g for g in (gl, gv) if g]


def raw_backward(x, theta, med, mode, g=None, g_bits=None, lb=R.LB, outs=(True, True, True)):
    """fgmm_eb_likelihood_backward -> (rc, dx, dtheta, dmed, guards); outs: which of the three are not NULL"""
    B, Cn, hw = x.shape
    gx, gt, gm = (Guarded(n) if want else None for want, n in zip(outs, (x.numel(), theta.numel(), med.numel())))
    gb = None if g_bits is None else np.ascontiguousarray(np.asarray(g_bits, np.float64))
    call = _lib.fgmm_eb_grad_call(x.data_ptr(), theta.data_ptr(), med.data_ptr(), B, Cn, hw, None if g is None else g.data_ptr(),
                                  None if gb is None else gb.ctypes.data, *(t.t.data_ptr() if t else None for t in (gx, gt, gm)), 0, 0)
    torch.cuda.current_stream().synchronize()
    rc = _lib.lib().fgmm_eb_likelihood_backward(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, C.byref(call), mode, lb)
    return rc, (gx.t.reshape(x.shape) if gx else None), (gt.t.reshape(theta.shape) if gt else None), (gm.t if gm else None), [t for t in (gx, gt, gm) if t]


def make(seed, B, Cn, hw):
    """the corpus' recipe at another shape -> x [B, C, hw], params {name: tensor}, theta [C, 58], med [C], g, all on the GPU; region (numpy)"""
    x, p, med, g, region = R.corpus(seed, (B, Cn, hw, 1))
    p = {n: dv(a) for n, a in p.items()}
    return dv(x.reshape(B, Cn, hw)), p, R.theta_of(p).contiguous(), dv(med), dv(g.reshape(B, Cn, hw)), region.reshape(B, Cn, hw)


def cpu(p):
    return {n: t.cpu() for n, t in p.items()}


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_entropy_bottleneck.npz")))


@pytest.fixture(scope="module")
def corpus(gold):
    """computed once, left unchanged: the fixture's inputs on the GPU and torch's float32 evaluation of the mirrored form there"""
    x, med, g = dv(gold["x"]), dv(gold["med"]), dv(gold["g"])
    p = {n: dv(gold["p." + n]) for n in R.NAMES}
    return dict(x=x, x3=x.reshape(2, R.C, -1), p=p, theta=R.theta_of(p).contiguous(), med=med, g=g, g3=g.reshape(2, R.C, -1),
                f32={m: R.forward(x, p, med, m) for m in (0, 1)}, b32={m: R.gradients(x, p, med, g, m) for m in (0, 1)})


# ---- a. the corpus: likelihood and gradients against the reference's float64 ------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_likelihood_on_the_corpus(gold, corpus, mode):
    rc, like, v, bits, nonf, guards = raw_forward(corpus["x3"], corpus["theta"], corpus["med"], mode)
    assert rc == 0 and all(g.intact() for g in guards)
    like64 = gold["like64_eval" if mode else "like64"].reshape(like.shape)
    region = gold["region"].reshape(like.shape)
    for r, name in enumerate(R.REGIONS):
        check_accuracy(f"likelihood mode {mode} {name}", like, corpus["f32"][mode]["out"], like64, mask=region == r, floor=LB32)
    med = corpus["med"].reshape(1, -1, 1)
    assert torch.equal(v, torch.round(corpus["x3"] - med) + med if mode else corpus["x3"])
    want_bits, want_nonf = R.bits_of(like.cpu().numpy())
    print("bits_q", bits, "host sum of the map", want_bits)
    assert np.array_equal(nonf, want_nonf) and (np.abs(bits - want_bits) <= like[0].numel()).all()  # log2's last place, per element


@pytest.mark.parametrize("mode", [0, 1])
def test_gradients_on_the_corpus(gold, corpus, mode):
    rc, dx, dtheta, dmed, guards = raw_backward(corpus["x3"], corpus["theta"], corpus["med"], mode, g=corpus["g3"])
    assert rc == 0 and all(g.intact() for g in guards)
    b32, region = corpus["b32"][mode], gold["region"].reshape(dx.shape)
    got = R.split_theta(dtheta.cpu().numpy())
    for n in R.NAMES:
        check_accuracy(f"mode {mode} d{n}", got[n], b32[n], gold[("d64_eval." if mode else "d64.") + n])
    if mode:
        assert not dx.any()
        check_accuracy("mode 1 dmed", dmed, b32["med"], gold["dmed64"])
    else:
        assert not dmed.any()
        for r, name in enumerate(R.REGIONS):
            check_accuracy(f"mode 0 dx {name}", dx, b32["x"].reshape(dx.shape), gold["dx64"], mask=region == r)


def test_g_bits_backward_equals_the_map_backward(corpus):
    x, theta, med = corpus["x3"], corpus["theta"], corpus["med"]
    gb = np.array([1.0, -0.37])
    for mode in (0, 1):
        _, like, _, _, _, _ = raw_forward(x, theta, med, mode)
        counts = (like > 0) & (like < float("inf"))
        g = torch.where(counts, -dv(gb.astype(np.float32)).reshape(-1, 1, 1) / (like * R.LN2F), torch.zeros_like(like))
        rc_a, *a, _ = raw_backward(x, theta, med, mode, g_bits=gb)
        rc_b, *b, _ = raw_backward(x, theta, med, mode, g=g.contiguous())
        assert rc_a == 0 and rc_b == 0 and all(torch.equal(p, q) for p, q in zip(a, b))
        assert a[1].abs().sum() > 0


# ---- b. shapes: every path of the walk, the slices' edges, both load widths ---------------------------------------------------------------
SHAPES = [(1, 3, 1), (3, 3, 21), (1, 1, 64), (5, 3, 13), (3, 3, 85), (1, 3, 256), (1, 3, 257), (3, 3, 5), (2, 1, 34), (4, 3, 64),
          (1, 3, S - 1), (2, 3, S // 2), (1, 3, S + 1), (1, 1, 2 * S + 1), (3, 3, 2 * S // 3 + 1)]


def test_shape_list_covers_what_it_claims():
    n = {B * hw for B, _, hw in SHAPES}
    assert {1, 63, 64, 65, 255, 256, 257, S - 1, S, S + 1, 2 * S + 1} <= n and (3, 3, 5) in SHAPES
    assert {1, 3} == {c for _, c, _ in SHAPES} and any(hw % 4 for _, _, hw in SHAPES) and any(hw % 4 == 0 and B > 1 for B, _, hw in SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(shape):
    B, Cn, hw = shape
    n = B * hw
    x, p, theta, med, g, _ = make(1000 + n + Cn, B, Cn, hw)
    flat = lambda t: t.permute(1, 0, 2).reshape(1, Cn, n).contiguous()  # noqa: E731  (the same elements as one item)
    for mode in (0, 1):
        rc, like, v, bits, nonf, guards = raw_forward(x, theta, med, mode)
        rc1, like1, v1, bits1, nonf1, _ = raw_forward(flat(x), theta, med, mode)
        assert rc == 0 and rc1 == 0 and all(t.intact() for t in guards)
        assert torch.equal(flat(like), like1) and torch.equal(flat(v), v1) and not torch.isnan(like).any()
        assert bits.sum() == bits1.sum() and nonf.sum() == nonf1.sum() == 0
        want_bits, _ = R.bits_of(like.cpu().numpy())
        assert (np.abs(bits - want_bits) <= Cn * hw).all()
        rc, dx, dtheta, dmed, guards = raw_backward(x, theta, med, mode, g=g)
        rc1, dx1, dtheta1, dmed1, _ = raw_backward(flat(x), theta, med, mode, g=flat(g))
        assert rc == 0 and rc1 == 0 and all(t.intact() for t in guards)
        assert torch.equal(flat(dx), dx1) and not torch.isnan(dtheta).any() and not torch.isnan(dmed).any()
        x4, g4 = x.reshape(B, Cn, hw, 1), g.reshape(B, Cn, hw, 1)
        b32 = R.gradients(x4, p, med, g4, mode)
        b64 = R.gradients(x4.cpu(), cpu(p), med.cpu(), g4.cpu(), mode, dtype=torch.float64)
        check_accuracy(f"{shape} mode {mode} likelihood", like, R.forward(x4, p, med, mode)["out"],
                       R.forward(x4.cpu(), cpu(p), med.cpu(), mode, dtype=torch.float64)["out"].numpy(), floor=LB32)
        check_accuracy(f"{shape} mode {mode} dtheta", dtheta, R.theta_of(b32), R.theta_of(b64).numpy())
        check_accuracy(f"{shape} mode {mode} dtheta as one item", dtheta1, R.theta_of(b32), R.theta_of(b64).numpy())
        if mode:
            check_accuracy(f"{shape} mode 1 dmed", dmed, b32["med"], b64["med"].numpy())
        else:
            check_accuracy(f"{shape} mode 0 dx", dx, b32["x"], b64["x"].numpy())


def test_same_call_twice_gives_the_same_bits():
    x, p, theta, med, g, _ = make(77, 3, 3, 1000)  # three partial rows per channel
    assert -(-3 * 1000 // S) > 1
    for mode, kw in ((0, dict(g=g)), (1, dict(g=g)), (0, dict(g_bits=[0.5, -2.0, 1.0]))):
        a, b = raw_backward(x, theta, med, mode, **kw), raw_backward(x, theta, med, mode, **kw)
        assert a[0] == 0 and all(torch.equal(s, t) for s, t in zip(a[1:4], b[1:4]))
        a, b = raw_forward(x, theta, med, mode), raw_forward(x, theta, med, mode)
        assert a[0] == 0 and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


def test_non_finite_values_stay_in_their_channel():
    x, p, theta, med, g, _ = make(78, 2, 3, 40)
    bad = x.clone()
    bad[0, 1, 7], bad[1, 1, 33] = float("nan"), float("inf")
    for lb in (R.LB, 0.0):  # (with a bound the +inf element's likelihood, 0, is raised to the bound: only the NaN is left out)
        rc, like, _, bits, nonf, _ = raw_forward(bad, theta, med, 0, lb=lb)
        _, want_nonf = R.bits_of(like.cpu().numpy())  # what the returned map says
        print("n_nonfinite", nonf, "from the map", want_nonf)
        assert rc == 0 and np.array_equal(nonf, want_nonf) and nonf[0] >= 1 and torch.isnan(like[0, 1, 7])
        assert nonf.sum() >= (2 if lb == 0 else 1)
        _, clean, _, _, _, _ = raw_forward(x, theta, med, 0, lb=lb)
        assert torch.equal(like[:, 0], clean[:, 0]) and torch.equal(like[:, 2], clean[:, 2])
        for kw in (dict(g=g), dict(g_bits=[1.0, 1.0])):
            rc, dx, dtheta, dmed, _ = raw_backward(bad, theta, med, 0, lb=lb, **kw)
            rc0, dx0, dtheta0, dmed0, _ = raw_backward(x, theta, med, 0, lb=lb, **kw)
            assert rc == 0 and rc0 == 0 and torch.equal(dtheta[0], dtheta0[0]) and torch.equal(dtheta[2], dtheta0[2]) and torch.equal(dx[:, 0], dx0[:, 0])


def test_every_null_output_subset(corpus):
    x, theta, med, g = corpus["x3"], corpus["theta"], corpus["med"], corpus["g3"]
    for mode in (0, 1):
        _, like, v, bits, nonf, _ = raw_forward(x, theta, med, mode)
        for wl, wv, host in itertools.product((True, False), repeat=3):
            rc, l2, v2, b2, n2, guards = raw_forward(x, theta, med, mode, like=wl, v=wv, host=host)
            assert rc == 0 and all(t.intact() for t in guards) and (not wl or torch.equal(l2, like)) and (not wv or torch.equal(v2, v))
            assert (np.array_equal(b2, bits) and np.array_equal(n2, nonf)) if host else ((b2 == -5).all() and (n2 == -5).all())
        _, *full, _ = raw_backward(x, theta, med, mode, g=g)
        for outs in itertools.product((True, False), repeat=3):
            rc, *got, guards = raw_backward(x, theta, med, mode, g=g, outs=outs)
            if not any(outs):
                assert rc == 1
                continue
            assert rc == 0 and all(t.intact() for t in guards) and all(t is None or torch.equal(t, f) for t, f in zip(got, full))


def test_refusals_leave_the_outputs_alone(corpus):
    x, theta, med, g = corpus["x3"], corpus["theta"], corpus["med"], corpus["g3"]
    B, Cn, hw = x.shape
    L, ctx, stream = _lib.lib(), _lib.ctx(0), torch.cuda.current_stream().cuda_stream
    like, v, dx, dtheta, dmed = Guarded(x.numel()), Guarded(x.numel()), Guarded(x.numel()), Guarded(theta.numel()), Guarded(med.numel())
    bits, nonf, gb = np.full(B, -5, np.int64), np.full(B, -5, np.int64), np.ones(B)
    good = dict(x=x.data_ptr(), theta=theta.data_ptr(), med=med.data_ptr(), B=B, C=Cn, hw=hw)
    bad_fields = [dict(x=None), dict(theta=None), dict(med=None), dict(B=0), dict(C=0), dict(hw=0), dict(B=-1), dict(hw=-4)]
    bad_args = [(2, R.LB), (-1, R.LB), (0, -1.0), (0, float("inf")), (1, float("nan"))]
    torch.cuda.synchronize()

    def fwd(fields, mode=0, lb=R.LB):
        call = _lib.fgmm_eb_call(**{**good, **fields}, like_out=like.t.data_ptr(), v_out=v.t.data_ptr(), bits_q=bits.ctypes.data, n_nonfinite=nonf.ctypes.data)
        return L.fgmm_eb_likelihood(ctx, stream, C.byref(call), mode, lb)

    def bwd(fields, mode=0, lb=R.LB, **over):
        kw = dict(g_like=g.data_ptr(), g_bits=gb.ctypes.data, dx=dx.t.data_ptr(), dtheta=dtheta.t.data_ptr(), dmed=dmed.t.data_ptr())
        call = _lib.fgmm_eb_grad_call(**{**good, **fields, **kw, **over})
        return L.fgmm_eb_likelihood_backward(ctx, stream, C.byref(call), mode, lb)

    for f in bad_fields:
        assert fwd(f) == 1 and bwd(f) == 1, f
        assert L.fgmm_last_error()
    for mode, lb in bad_args:
        assert fwd({}, mode, lb) == 1 and bwd({}, mode, lb) == 1, (mode, lb)
    assert bwd({}, dx=None, dtheta=None, dmed=None) == 1
    assert bwd({}, g_like=None, g_bits=None) == 1
    bad_gb = np.array([1.0, float("inf")])
    assert bwd({}, g_like=None, g_bits=bad_gb.ctypes.data) == 1
    torch.cuda.synchronize()
    assert all(t.untouched() for t in (like, v, dx, dtheta, dmed)) and (bits == -5).all() and (nonf == -5).all()
    assert fwd({}) == 0 and bwd({}) == 0 and not any(t.untouched() for t in (like, v, dx, dtheta, dmed)) and all(t.intact() for t in (like, v, dx, dtheta, dmed))


# ---- c. the caller's stream ---------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_with_a_pending_producer(streams, delay):  # noqa: F811
    s1, s2, third = streams
    x, p, theta, med, g, _ = make(91, 2, 3, 1500)
    x_d, _, theta_d, med_d, g_d, _ = make(92, 2, 3, 1500)
    true, decoy = [x, theta, med, g], [x_d, theta_d, med_d, g_d]
    _, like_w, _, bits_w, _, _ = raw_forward(x, theta, med, 0)
    _, *grads_w, _ = raw_backward(x, theta, med, 0, g=g)
    assert not torch.equal(like_w, raw_forward(x_d, theta_d, med_d, 0)[1])
    with pending(s1, delay, true, decoy) as t:
        rc, like, v, bits, _, _ = raw_forward(t[0], t[1], t[2], 0)
        like_3, v_3 = snapshot(third, [like, v])
    assert rc == 0 and torch.equal(like_3, like_w) and torch.equal(v_3, x) and np.array_equal(bits, bits_w)
    with pending(s2, delay, true, decoy) as t:
        rc, *grads, _ = raw_backward(t[0], t[1], t[2], 0, g=t[3])
        grads_3 = snapshot(third, grads)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(grads_3, grads_w))


# ---- d. the module ------------------------------------------------------------------------------------------------------------------------
def module_from(gold):
    eb = EntropyBottleneck(R.C)
    eb.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("sd.")}, strict=True)
    return eb.to(DEV)


def test_module_eval_mode_and_its_gradients(gold, corpus):
    eb = module_from(gold).eval()
    x = corpus["x"].clone().requires_grad_(True)
    outputs, like = eb(x)
    assert outputs.shape == x.shape == like.shape
    _, like_raw, v_raw, bits_raw, nonf_raw, _ = raw_forward(corpus["x3"], corpus["theta"], corpus["med"], 1)
    assert torch.equal(like.reshape(like_raw.shape), like_raw) and torch.equal(outputs.reshape(v_raw.shape), v_raw) and not outputs.requires_grad
    (like * corpus["g"]).sum().backward()
    _, _, dtheta, dmed, _ = raw_backward(corpus["x3"], corpus["theta"], corpus["med"], 1, g=corpus["g3"])
    want = R.split_theta(dtheta.cpu().numpy())
    for n in R.NAMES:
        assert np.array_equal(getattr(eb, n).grad.cpu().numpy(), want[n]), n
    q = eb.quantiles.grad
    assert torch.equal(q[:, 0, 1], dmed) and not q[:, 0, 0].any() and not q[:, 0, 2].any() and x.grad is None
    eb.zero_grad()
    out2, bits, nonf = eb.rate_bits(corpus["x"], return_nonfinite=True)
    assert torch.equal(out2, outputs) and bits.dtype == torch.float64 and bits.device.type == "cuda"
    assert np.array_equal(bits.detach().cpu().numpy(), bits_raw * 2.0 ** -32) and np.array_equal(nonf.numpy(), nonf_raw)
    w = torch.tensor([0.25, -1.5], dtype=torch.float64, device=DEV)
    (bits * w).sum().backward()
    _, _, dtheta, dmed, _ = raw_backward(corpus["x3"], corpus["theta"], corpus["med"], 1, g_bits=w.cpu().numpy())
    assert torch.equal(torch.cat([getattr(eb, n).grad.reshape(R.C, -1) for n in R.NAMES], 1), dtheta)
    assert torch.equal(eb.quantiles.grad[:, 0, 1], dmed)


def test_module_training_mode_and_its_gradients(gold, corpus):
    eb = module_from(gold).train()
    x = corpus["x"].clone().requires_grad_(True)
    torch.manual_seed(11)
    outputs, like = eb(x)
    noise = (outputs - x).detach()
    assert float(noise.min()) >= -0.5 and float(noise.max()) <= 0.5 and float(noise.std()) > 0.2
    v, block = eb.likelihood(outputs.detach())  # the building block on the returned outputs: the same map, bit for bit
    assert torch.equal(block, like) and torch.equal(v, outputs)
    (like * corpus["g"]).sum().backward()
    x3 = outputs.detach().reshape(2, R.C, -1).contiguous()
    _, dx, dtheta, _, _ = raw_backward(x3, corpus["theta"], corpus["med"], 0, g=corpus["g3"])
    assert torch.equal(x.grad.reshape(dx.shape), dx)
    assert torch.equal(torch.cat([getattr(eb, n).grad.reshape(R.C, -1) for n in R.NAMES], 1), dtheta)
    assert eb.quantiles.grad is None or not eb.quantiles.grad.any()  # the noised path does not see the medians
    torch.manual_seed(11)
    out2, bits = eb.rate_bits(corpus["x"])
    assert torch.equal(out2, outputs.detach()) and bits.shape == (2,)
    assert torch.equal(eb(corpus["x"], training=False)[0], eb.eval()(corpus["x"])[0])


@pytest.mark.parametrize("quantizer", ["noise", "ste"])
def test_hyper_latent_codec_forward_against_its_parts(gold, corpus, quantizer):
    torch.manual_seed(5)
    eb = module_from(gold).eval()
    h_a, h_s = torch.nn.Conv2d(4, R.C, 1).to(DEV), torch.nn.Conv2d(R.C, 3, 1).to(DEV)
    codec = HyperLatentCodec(entropy_bottleneck=eb, h_a=h_a, h_s=h_s, quantizer=quantizer).eval()
    y = torch.randn(2, 4, 6, 10, device=DEV) * 20
    out = codec(y)
    z = h_a(y)
    z_hat, like = eb(z)
    assert torch.equal(out["likelihoods"]["z"], like) and torch.equal(z_hat, torch.round(z - eb._get_medians()) + eb._get_medians())
    assert torch.allclose(out["params"], h_s(z_hat), atol=1e-5)
    out["likelihoods"]["z"].log2().sum().neg().backward()
    assert all(getattr(eb, n).grad is not None and torch.isfinite(getattr(eb, n).grad).all() for n in R.NAMES)
    enc = codec.compress(y)  # the fast path: this class's coder() on its own tables
    assert torch.allclose(codec.decompress(enc["strings"], enc["shape"])["params"], enc["params"], atol=1e-6)
    assert enc["strings"][0] == eb.coder().compress(z)
