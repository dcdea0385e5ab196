"""GPU (-m gpu): the entropy model's forward() on the GPU (include/flashgmm_amd.h section 3g; fgmm_like.hip, fgmm_like.cpp) - the
likelihood, its rate and its gradients through ``GaussianMixtureConditional.forward`` / ``rate_bits`` / ``likelihood``, the two C entry
points through ctypes, and ``GaussianMixtureConditionalLatentCodec.forward``.

Accuracy is never an absolute figure here.  The yardstick is the same formula evaluated with torch float32 operations on the GPU
(tests/like_ref.py): per region and quantity E = max |x32 - x64| / max(|x64|, floor) against float64 - the fixture's values from the
reference's own class on the corpus, elsewhere the restated forward and autograd through it (R.forward, R.reference_gradients), which
tests/test_likelihood_cpu.py ties to that class - once for torch (E_ref) and once for the kernel (E_k), and
E_k <= 2 * E_ref + 2^-23 is required: two correct binary32 evaluations of one formula that differ in their erfc / exp may each be off by
their own rounding, and the formula's cancellation amplifies both alike.  The floor is the likelihood bound for likelihoods, 1e-6 times
the region's largest float64 magnitude for a gradient.  Every figure is printed before it is asserted (run with -s to see them)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec
from test_gpu_streams import delay, pending, snapshot, streams  # noqa: F401  (the stream case runs in that module's manner, on its helpers)
from tests import like_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB32 = R.f32(R.LB)
NAMES = ("y", "scales", "means", "weights")


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g10_likelihood.npz")))


@pytest.fixture(scope="module")
def gmc():
    return GaussianMixtureConditional(K=4).eval()


@pytest.fixture(scope="module")
def corpus_ref(gold):
    """computed once, left unchanged: torch's float32 evaluation on the GPU of the fixture's inputs, with rounding (forward only, and
    its float64 restatement on the CPU) and without (forward and backward at the fixture's g; their float64 values are the fixture's)"""
    cpu = [torch.from_numpy(gold[k]) for k in NAMES]
    gpu = [t.to(DEV) for t in cpu]
    g = torch.from_numpy(gold["g"])
    f32 = R.forward(*gpu, rnd=False)
    return dict(gpu=gpu, g=g.to(DEV), eval64=R.forward(*cpu, rnd=True, dtype=torch.float64)["out"].numpy(),
                eval32=R.forward(*gpu, rnd=True)["out"].cpu().numpy(), like32=f32["out"].cpu().numpy(),
                b32={k: v.cpu().numpy() for k, v in R.backward(f32, g.to(DEV)).items()})


def err(x, x64, floor, mask=None):
    e = np.abs(x.astype(np.float64) - x64) / np.maximum(np.abs(x64), floor)
    return float(e[mask].max()) if mask is not None else float(e.max())


def check_accuracy(what, got, ref32, x64, mask=None, floor=None):
    """E_k <= 2 * E_ref + 2^-23 on the rows of `mask` (see the module's docstring); floor None: a gradient's, from the region itself"""
    if mask is not None and not mask.any():
        return
    if floor is None:
        floor = max(1e-6 * float(np.abs(x64[mask] if mask is not None else x64).max()), 1e-300)
    e_ref, e_k = err(ref32, x64, floor, mask), err(got, x64, floor, mask)
    print(f"accuracy {what:28s} E_ref {e_ref:.3e}  E_k {e_k:.3e}  ratio {e_k / e_ref if e_ref else float('inf') if e_k else 1.0:.3f}")
    assert e_k <= 2.0 * e_ref + 2.0 ** -23, (what, e_ref, e_k)


def make(seed, B, M, h, w, dtype=torch.float32):
    """typical inputs of a given shape (region (a)'s recipe), some sigma below the scale bound -> y, scales, means, weights, g on the GPU"""
    rng = np.random.default_rng(seed)
    n = (B, 4, M, h, w)
    sg = (np.exp(rng.uniform(-3, 2.5, (B, 1, M, h, w))) * rng.uniform(0.5, 2.0, n)).astype(np.float32)
    base = rng.standard_normal((B, M, h, w)) * 4
    mu = (base[:, None] + rng.standard_normal(n) * sg * 1.5).astype(np.float32)
    y = (base + rng.standard_normal((B, M, h, w)) * sg.mean(1) * 1.5).astype(np.float32)
    lg = rng.standard_normal(n)
    pi = (np.exp(lg) / np.exp(lg).sum(1, keepdims=True)).astype(np.float32)
    g = (rng.standard_normal((B, M, h, w)) * np.exp(rng.uniform(-2, 2, (B, M, h, w)))).astype(np.float32)
    planes = [dv(a.reshape(B, 4 * M, h, w)).to(dtype) for a in (sg, mu, pi)]
    return [dv(y)] + planes + [dv(g)]


def grads_through_map(gmc, y, s, m, w, g, rnd=False):
    """-> (v, likelihood, [dy, dscales, dmeans, dweights]) of one ``likelihood`` call and its backward at g (dy None with rounding).
    The leaves are the tensors themselves (detached, not cloned: a clone would be a fresh, aligned and dense allocation, and the call
    would no longer see the addresses and strides the test built)"""
    leaves = [t.detach().requires_grad_(True) for t in (y, s, m, w)]
    v, like = gmc.likelihood(*leaves, round=rnd)
    like.backward(g)
    return v.detach(), like.detach(), [t.grad for t in leaves]


# ---- the two entry points through ctypes ---------------------------------------------------------------------------------------------
def _fill(it, y, s, m, w, K=4, flags=0, size=None):
    M, hw, sk, sc = (tuple(size) + (size[0] * size[1], size[1]))[:4] if size is not None else (y.shape[0], y[0].numel(), y.numel(), y[0].numel())
    it.y = y.data_ptr()
    it.params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), sk, sc, {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}[s.dtype], flags)
    it.M, it.K, it.hw = M, K, hw


def raw_forward(items, rnd, want_map=True, sb=R.SB, lb=R.LB, K=4, flags=0, fill=None, outs=None, sizes=None):
    """fgmm_gmc_likelihood_batch on items (y [M, h, w], scales, means, weights [4M, h, w]), all contiguous device tensors ->
    (rc, [(like, v, bits_q, n_nonfinite)]); `fill`: the outputs are pre-filled with it (refusals must leave them alone); `outs`: per
    item the caller's own (like, v) tensors, None for a NULL output; `sizes`: per item (M, hw) or (M, hw, stride_k, stride_c) in place of the tensors' own"""
    arr = (_lib.fgmm_like_item * len(items))()
    given, outs = outs, []
    for i, (it, (y, s, m, w)) in enumerate(zip(arr, items)):
        _fill(it, y, s, m, w, K, flags, sizes[i] if sizes else None)
        if given is not None:
            like, v = given[i]
            it.like_out, it.v_out = (t.data_ptr() if t is not None else None for t in (like, v))
            outs.append((like, v))
            continue
        like, v = (torch.empty_like(y, dtype=torch.float32) if fill is None else torch.full_like(y, fill, dtype=torch.float32) for _ in range(2))
        it.like_out, it.v_out = (like.data_ptr() if want_map else None), v.data_ptr()
        outs.append((like, v))
    if fill is not None:
        torch.cuda.current_stream().synchronize()
    rc = _lib.lib().fgmm_gmc_likelihood_batch(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, arr, len(items), int(rnd), sb, lb)
    return rc, [(like, v, int(it.bits_q), int(it.n_nonfinite)) for it, (like, v) in zip(arr, outs)]


def raw_backward(items, gs, rnd, g_bits=None, sb=R.SB, lb=R.LB, outs=None, sizes=None):
    """fgmm_gmc_likelihood_backward_batch -> (rc, [(dy, dscales, dmeans, dweights)]); gs: the items' g_like, or None with g_bits;
    `outs`: per item the caller's own four tensors, None for a NULL output; `sizes`: per item (M, hw) or (M, hw, stride_k, stride_c) in place of the tensors' own"""
    arr = (_lib.fgmm_like_grad_item * len(items))()
    given, outs = outs, []
    for i, (it, (y, s, m, w)) in enumerate(zip(arr, items)):
        _fill(it, y, s, m, w, size=sizes[i] if sizes else None)
        o = given[i] if given is not None else [torch.empty_like(y)] + [torch.empty(s.shape, dtype=torch.float32, device=DEV) for _ in range(3)]
        it.dy, it.dscales, it.dmeans, it.dweights = (t.data_ptr() if t is not None else None for t in o)
        if gs is not None:
            it.g_like = gs[i].data_ptr()
        else:
            it.g_bits = g_bits[i]
        outs.append(o)
    rc = _lib.lib().fgmm_gmc_likelihood_backward_batch(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, arr, len(items), int(rnd), sb, lb)
    return rc, outs


# ---- a. forward, evaluation mode, the fixture's layout -------------------------------------------------------------------------------
def test_forward_eval_on_the_corpus(gmc, corpus_ref):
    y, s, m, w = corpus_ref["gpu"]
    outputs, like = gmc(y, s, m, w)
    assert torch.equal(outputs, torch.round(y)) and like.shape == y.shape and like.dtype == torch.float32
    like = like.cpu().numpy()
    assert np.all(like[R.region_mask("c")] == np.float32(LB32))
    for name in R.REGIONS:
        check_accuracy(f"likelihood eval ({name})", like, corpus_ref["eval32"], corpus_ref["eval64"], R.region_mask(name), LB32)


# ---- b. every load path ---------------------------------------------------------------------------------------------------------------
def offset_views(t):
    """the same values at addresses one element past an aligned one: the wide loads are refused"""
    return [x.new_empty(x.numel() + 1)[1:].view(x.shape).copy_(x) for x in t]


@pytest.mark.parametrize("case", ["hw255", "M3_hw768", "B3_hw64", "offset_hw256", "hw64_offset"])
def test_forward_and_backward_on_every_float32_load_path(gmc, case):
    B, M, h, w = {"hw255": (1, 4, 15, 17), "M3_hw768": (1, 3, 24, 32), "B3_hw64": (3, 2, 8, 8), "offset_hw256": (1, 8, 16, 16), "hw64_offset": (2, 3, 8, 8)}[case]
    t = make(4100 + len(case), B, M, h, w)
    if "offset" in case:
        t = offset_views(t)
        assert all(x.data_ptr() % 16 == 4 for x in t)
    y, s, m, wt, g = t
    cpu = [x.cpu() for x in t]
    for rnd in (True, False):
        f64, f32 = R.forward(*cpu[:4], rnd=rnd, dtype=torch.float64), R.forward(y, s, m, wt, rnd=rnd)
        v, like, grads = grads_through_map(gmc, y, s, m, wt, g, rnd)
        assert torch.equal(v, torch.round(y) if rnd else y) and (grads[0] is None) == rnd
        check_accuracy(f"{case} likelihood rnd={int(rnd)}", like.cpu().numpy(), f32["out"].cpu().numpy(), f64["out"].numpy(), floor=LB32)
        b64, b32 = R.reference_gradients(*cpu, rnd=rnd)[1], R.backward(f32, g)
        for name, got in zip(R.GRADS, grads):
            if got is not None:
                check_accuracy(f"{case} {name} rnd={int(rnd)}", got.cpu().numpy(), b32[name].cpu().numpy(), b64[name].numpy())
    # the stacked call is its items one by one
    if B > 1:
        _, like_all = gmc(y, s, m, wt)
        for i in range(B):
            assert torch.equal(gmc(y[i:i + 1], s[i:i + 1], m[i:i + 1], wt[i:i + 1])[1], like_all[i:i + 1])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
# hw = 256 (4 per lane on the linear grid: 8 would leave it), 264 (8 per lane, tiled grid), 252 (4 per lane, tiled), 512 (8 per lane, linear)
@pytest.mark.parametrize("shape", [(1, 4, 16, 16), (1, 4, 12, 22), (1, 4, 14, 18), (2, 2, 16, 32)])
def test_two_byte_planes_equal_float32_planes_holding_the_widened_values(gmc, dtype, shape):
    y, s, m, wt, g = make(4200 + shape[2], *shape, dtype=dtype)
    assert s.dtype == dtype
    wide = [x.to(torch.float32) for x in (s, m, wt)]
    for rnd in (True, False):
        v2, like2, grads2 = grads_through_map(gmc, y, s, m, wt, g, rnd)
        v4, like4, grads4 = grads_through_map(gmc, y, *wide, g, rnd)
        assert torch.equal(v2, v4) and torch.equal(like2.view(torch.int32), like4.view(torch.int32))
        for name, a, b in zip(R.GRADS, grads2, grads4):
            if a is not None:
                assert a.dtype == (dtype if name != "dy" else torch.float32) and b.dtype == torch.float32
                assert torch.equal(a, b.to(a.dtype)), (name, rnd)  # (the kernel's float32 planes, rounded once to the inputs' dtype)
        # the float32 gradient planes themselves, and the sums, through ctypes: bit for bit
        items2 = [(y[i], s[i], m[i], wt[i]) for i in range(shape[0])]
        items4 = [(y[i], wide[0][i], wide[1][i], wide[2][i]) for i in range(shape[0])]
        (rc2, f2), (rc4, f4) = raw_forward(items2, rnd), raw_forward(items4, rnd)
        assert rc2 == 0 and rc4 == 0
        for (l2, _, b2, n2), (l4, _, b4, n4) in zip(f2, f4):
            assert torch.equal(l2.view(torch.int32), l4.view(torch.int32)) and b2 == b4 and n2 == n4 == 0
        (rc2, o2), (rc4, o4) = raw_backward(items2, list(g), rnd), raw_backward(items4, list(g), rnd)
        assert rc2 == 0 and rc4 == 0
        for a, b in zip(o2, o4):
            assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
        (rc2, o2), (rc4, o4) = raw_backward(items2, None, rnd, g_bits=[1.5, -0.25]), raw_backward(items4, None, rnd, g_bits=[1.5, -0.25])
        assert rc2 == 0 and rc4 == 0
        for a, b in zip(o2, o4):
            assert all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))
    # and against float64 on the widened values, as everywhere
    cpu = [y.cpu()] + [x.cpu() for x in wide]
    f64, f32 = R.forward(*cpu, rnd=True, dtype=torch.float64), R.forward(y, *wide, rnd=True)
    check_accuracy(f"{dtype} {shape} likelihood", gmc(y, s, m, wt)[1].cpu().numpy(), f32["out"].cpu().numpy(), f64["out"].numpy(), floor=LB32)


# ---- c. training mode -----------------------------------------------------------------------------------------------------------------
def test_training_mode_adds_noise_and_prices_the_noised_values(corpus_ref):
    y, s, m, w = corpus_ref["gpu"]
    gmc = GaussianMixtureConditional(K=4).train()
    torch.manual_seed(31)
    outputs, like = gmc(y, s, m, w)
    d = (outputs.double() - y.double())
    assert float(d.min()) >= -0.5 and float(d.max()) <= 0.5 and float(d.std()) > 0.2
    assert torch.equal(like, gmc.likelihood(outputs, s, m, w, round=False)[1])
    assert torch.equal(like, gmc(outputs, s, m, w, training=False)[1]) is False  # (rounding changes the values)
    torch.manual_seed(31)
    assert torch.equal(gmc(y, s, m, w, training=True)[0], outputs)


# ---- d. backward through the likelihood map, on the corpus ------------------------------------------------------------------------------
def test_backward_through_the_map_on_the_corpus(gmc, gold, corpus_ref):
    y, s, m, w = corpus_ref["gpu"]
    v, like, grads = grads_through_map(gmc, y, s, m, w, corpus_ref["g"])
    assert torch.equal(v, y)
    like = like.cpu().numpy()
    keep = ~R.near_bound(gold["L64"])  # the 1 % rule (tests/test_likelihood_cpu.py checks the share)
    assert keep.mean() >= 0.99
    for name in R.REGIONS:
        check_accuracy(f"likelihood v=y ({name})", like, corpus_ref["like32"], gold["like64"], R.region_mask(name) & keep, LB32)
    for gname, got in zip(R.GRADS, grads):
        got, want = got.cpu().numpy(), gold[gname + "64"]
        rows = keep if gname == "dy" else np.tile(keep, (1, 4, 1, 1))
        for name in R.REGIONS:
            mask = (R.region_mask(name) if gname == "dy" else R.plane_mask(name)) & rows
            check_accuracy(f"{gname} ({name})", got, corpus_ref["b32"][gname], want, mask)
        # the pass-through decisions: where the reference's gradient is zero the kernel's is; where it is not, the kernel's is zero only
        # where binary32 itself gives zero (exp underflows in region (c), phi(xu) - phi(xl) cancels to nothing in region (f)): there
        # torch's float32 evaluation of the formula is zero too, and a zero is no decision
        assert np.all(got[rows & (want == 0)] == 0), gname
        live = rows & (want != 0)
        assert np.array_equal(got[live] == 0, corpus_ref["b32"][gname][live] == 0) and (got[live] != 0).mean() > 0.8, gname
    # region (d): the hit component's mean gets exactly nothing, and dy is the ascending sum of the others' shares
    dmu = grads[2].cpu()
    mu, yc = corpus_ref["gpu"][2].cpu(), y.cpu()
    hit = (mu.view(1, 4, 8, 16, 16) == yc.unsqueeze(1)) & torch.from_numpy(R.region_mask("d")).unsqueeze(1)
    assert int(hit.sum()) >= 256 and torch.all(dmu.view(1, 4, 8, 16, 16)[hit] == 0)
    dy = torch.zeros_like(yc)
    for k in range(4):
        dy = dy + (-dmu.view(1, 4, 8, 16, 16)[:, k])
    assert torch.equal(dy, grads[0].cpu())
    # evaluation mode: nothing arrives at the inputs
    leaf = y.detach().clone().requires_grad_(True)
    planes = [t.detach().clone().requires_grad_(True) for t in (s, m, w)]
    gmc(leaf, *planes)[1].backward(corpus_ref["g"])
    assert leaf.grad is None or not leaf.grad.any()
    assert all(p.grad is not None and p.grad.any() for p in planes)


# ---- e. the rate ----------------------------------------------------------------------------------------------------------------------
def test_rate_is_the_integer_sum_of_the_map(gmc, corpus_ref):
    y, s, m, w = corpus_ref["gpu"]
    item = lambda yy, mm=m: [(yy[0], s[0], mm[0], w[0])]  # noqa: E731
    rc, [(like, v, bits_q, nonfinite)] = raw_forward(item(y), True)
    assert rc == 0 and nonfinite == 0 and torch.equal(v, torch.round(y[0]))
    n = like.numel()
    want = float((-np.log2(like.cpu().numpy().astype(np.float64))).sum())
    got = bits_q * 2.0 ** -32
    print(f"rate: bits_q {bits_q}  = {got!r} bits, host float64 sum {want!r}, difference {got - want:.3e}")
    assert abs(got - want) <= n * 2.0 ** -33 + 1e-12 * abs(want)
    for _ in range(2):  # three runs, one integer
        assert raw_forward(item(y), True)[1][0][2] == bits_q
    # ... without the map, and through the public call
    assert raw_forward(item(y), True, want_map=False)[1][0][2] == bits_q
    outputs, bits, nf = gmc.rate_bits(y, s, m, w, return_nonfinite=True)
    assert torch.equal(outputs, torch.round(y)) and bits.dtype == torch.float64 and bits.shape == (1,) and float(bits[0]) == got and nf.tolist() == [0]
    # NaN in two latents: left out and counted, everything else unchanged
    at = [(1, 3, 5), (6, 10, 2)]
    y_nan, m_nan = y.clone(), m.clone()
    for c, i, j in at:
        y_nan[0, c, i, j] = float("nan")
        m_nan[0, c, i, j] = float("nan")  # (component 0's mean of the same latents)
    _, [(like_n, _, bits_n, nf_n)] = raw_forward(item(y_nan), True)
    _, [(like_m, _, bits_m, nf_m)] = raw_forward(item(y, m_nan), True)
    assert nf_n == 2 and nf_m == 2 and bits_n == bits_m
    hole = torch.zeros_like(like, dtype=torch.bool)
    for c, i, j in at:
        hole[c, i, j] = True
    for lk in (like_n, like_m):
        assert torch.all(torch.isnan(lk[hole])) and torch.equal(lk[~hole], like[~hole])
    # the sum over the others: the first run's minus the two terms, which the host's log2 may round one unit apart from the device's
    terms = [int(np.rint(-np.log2(float(like[c, i, j])) * 2.0 ** 32)) for c, i, j in at]
    assert abs(bits_n - (bits_q - sum(terms))) <= 2


# ---- f. backward through rate_bits ------------------------------------------------------------------------------------------------------
def test_backward_through_rate_bits_is_the_map_backward_at_its_own_gradient():
    gmc = GaussianMixtureConditional(K=4).train()
    y, s, m, w, _ = make(4600, 2, 3, 16, 16)
    gb = [1.5, -0.375]
    leaves = [t.detach().clone().requires_grad_(True) for t in (y, s, m, w)]
    torch.manual_seed(5)
    outputs, bits = gmc.rate_bits(*leaves)
    assert bits.requires_grad and bits.shape == (2,)
    (bits * torch.tensor(gb, dtype=torch.float64, device=DEV)).sum().backward()
    leaves2 = [t.detach().clone().requires_grad_(True) for t in (y, s, m, w)]
    torch.manual_seed(5)
    outputs2, like = gmc(*leaves2)
    assert torch.equal(outputs, outputs2)
    g = torch.stack([R.g_from_bits(like[i].detach().cpu(), gb[i]) for i in range(2)]).to(DEV)  # torch, binary32, correctly rounded
    like.backward(g)
    for a, b in zip(leaves, leaves2):
        assert a.grad is not None and torch.equal(a.grad.view(torch.int32), b.grad.view(torch.int32))
    assert float(bits.detach().sum()) == pytest.approx(float((-torch.log2(like.detach().double())).sum()), rel=1e-9)


# ---- g. through ctypes: a batch is its items -------------------------------------------------------------------------------------------
def test_two_items_of_different_shapes_in_one_call_equal_each_alone():
    a, b = make(4700, 1, 5, 12, 20), make(4701, 1, 2, 8, 8)
    items = [tuple(t[0] for t in a[:4]), tuple(t[0] for t in b[:4])]
    gs = [a[4][0], b[4][0]]
    for rnd in (True, False):
        rc, both = raw_forward(items, rnd)
        assert rc == 0
        for i in range(2):
            rc, [alone] = raw_forward(items[i:i + 1], rnd)
            assert rc == 0 and torch.equal(alone[0], both[i][0]) and torch.equal(alone[1], both[i][1]) and alone[2:] == both[i][2:]
        rc, both = raw_backward(items, gs, rnd)
        assert rc == 0
        for i in range(2):
            rc, [alone] = raw_backward(items[i:i + 1], gs[i:i + 1], rnd)
            assert rc == 0 and all(torch.equal(p, q) for p, q in zip(alone, both[i]))


# ---- h. the caller's-stream contract ---------------------------------------------------------------------------------------------------
def test_forward_and_backward_with_a_pending_producer(gmc, streams, delay):  # noqa: F811
    s1, s2, third = streams
    true, decoy = make(4800, 2, 4, 16, 16), make(4801, 2, 4, 16, 16)
    _, like_w, grads_w = grads_through_map(gmc, *true, rnd=False)
    _, bits_w = gmc.rate_bits(*true[:4], training=False)
    assert not torch.equal(like_w, grads_through_map(gmc, *decoy, rnd=False)[1])
    with pending(s1, delay, true, decoy) as t:
        outputs, like = gmc(*t[:4], training=False)
        like_3, out_3 = snapshot(third, [like, outputs])
        bits = gmc.rate_bits(*t[:4], training=False)[1]
    assert torch.equal(like_3, gmc(*true[:4], training=False)[1]) and torch.equal(out_3, torch.round(true[0])) and torch.equal(bits, bits_w)
    with pending(s2, delay, true, decoy) as t:
        items = [tuple(x[i] for x in t[:4]) for i in range(2)]
        rc, outs = raw_backward(items, list(t[4]), False)
        outs_3 = snapshot(third, [o for item in outs for o in item])
    assert rc == 0
    want = [x.to(torch.float32) for x in grads_w]
    for i in range(2):
        assert all(torch.equal(o, wg[i].reshape(o.shape)) for o, wg in zip(outs_3[4 * i:4 * i + 4], want))


# ---- i. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(gmc):
    y, s, m, w, g = make(4900, 1, 4, 8, 8)
    item = [(y[0], s[0], m[0], w[0])]
    for kw in (dict(K=3), dict(flags=_lib.FGMM_PARAMS_LOGITS), dict(sb=0.0), dict(sb=-1.0), dict(lb=-1e-9), dict(lb=float("nan"))):
        rc, [(like, v, _, _)] = raw_forward(item, True, fill=-7.0, **kw)
        torch.cuda.synchronize()
        assert rc == 1 and torch.all(like == -7.0) and torch.all(v == -7.0), kw
    arr = (_lib.fgmm_like_grad_item * 1)()
    _fill(arr[0], *item[0])
    arr[0].g_like = g.data_ptr()
    assert _lib.lib().fgmm_gmc_likelihood_backward_batch(_lib.ctx(0), None, arr, 1, 0, R.SB, R.LB) == 1  # every output null
    with pytest.raises(RuntimeError):
        GaussianMixtureConditional(K=3)(y, s[:, :12], m[:, :12], w[:, :12])
    with pytest.raises(RuntimeError):
        gmc(y.double(), s, m, w)
    with pytest.raises(RuntimeError):
        gmc(y[:, :3], s, m, w)
    with pytest.raises(RuntimeError):
        gmc(y, s, m[:, :8], w)
    with pytest.raises(RuntimeError):
        gmc.rate_bits(y, s, m.double(), w)
    with pytest.raises(ValueError):
        GaussianMixtureConditional(K=4, scale_bound=0.0)


# ---- j. the latent codec ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantizer", ["noise", "weighted_mean_ste"])
def test_latent_codec_forward_is_the_composition_of_its_parts(quantizer):
    M, h, w = 6, 8, 12
    rng = np.random.default_rng(5000)
    y = dv((rng.standard_normal((2, M, h, w)) * 3).astype(np.float32))
    ctx = rng.standard_normal((2, 12 * M, h, w)).astype(np.float32)
    ctx[:, :4 * M] = np.exp(ctx[:, :4 * M])  # scales
    ctx = dv(ctx).requires_grad_(True)
    codec = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer).to(DEV)
    gmc = codec.gaussian_mixture_conditional
    assert gmc.scale_bound == 0.11 and gmc.likelihood_bound == 1e-9

    def parts(training):
        scales, means, logits = ctx.chunk(3, 1)
        weights = torch.softmax(logits.reshape(2, 4, M, h, w), dim=1).reshape(2, 4 * M, h, w)
        if quantizer == "noise":
            return gmc(y, scales, means, weights, training=training)
        ws = (means.view(2, 4, M, h, w) * weights.view(2, 4, M, h, w)).sum(1)
        d = y - ws
        rel = (means.view(2, 4, M, h, w) - ws.unsqueeze(1)).reshape(2, 4 * M, h, w)
        return gmc((torch.round(d) - d).detach() + d + ws, scales, rel, weights, training=training)

    for training in (False, True):
        codec.train(training)
        torch.manual_seed(77)
        out = codec(y, ctx)
        torch.manual_seed(77)
        y_hat, like = parts(training)
        assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y"}
        assert torch.equal(out["y_hat"], y_hat) and torch.equal(out["likelihoods"]["y"], like)
    # the rate term of a training loss reaches the parameter network's output
    codec.train()
    (-torch.log2(codec(y, ctx)["likelihoods"]["y"])).sum().backward()
    assert ctx.grad is not None and torch.isfinite(ctx.grad).all() and ctx.grad.abs().sum() > 0
