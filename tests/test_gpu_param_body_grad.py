"""GPU: the hidden layers' gradients on the matrix cores (header section 2d; fgmm_hidden_grad.hip, ops.pointwise_layer, the checkerboard
codec's forward()).  Bars: bit for bit oracle.head_params' fmaf chains - over W^T and gz; per slice over the positions, then binary32 adds -
at every block height; the float64 bounds; float64 autograd."""
import copy

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from flashgmm_amd.ops import pointwise_layer
from tests import ckbd_ctx_grad_ref as G
from tests import head_ref as H
from tests.test_gpu_param_body import LEAKY, NONE, RELU, create, dv

pytestmark = pytest.mark.gpu
F32 = np.float32
SLOPE = 0.01
ACT_NAME = {NONE: "none", LEAKY: "leaky_relu", RELU: "relu"}


def ok(rc):
    assert rc == 0, _lib.lib().fgmm_last_error()


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def gz_ref(gy, out, act):
    """section 2d's three rules, in binary32"""
    if act == NONE:
        return gy
    return np.where(out > 0, gy, gy * F32(SLOPE) if act == LEAKY else F32(0)).astype(F32)


def make(seed, c_a, c_b, c_out, hw, n):
    r = np.random.default_rng(seed)
    g = lambda *s: r.standard_normal(s).astype(F32)
    return g(c_out, c_a + c_b), g(c_out), g(n, c_a, hw), g(n, c_b, hw), g(n, c_out, hw), g(n, c_out, hw)  # W, b, xa, xb, gy, out


def pack(W, b, c_a, transposed):
    L, (c_out, c_in) = _lib.lib(), W.shape
    floats = L.fgmm_hidden_packed_floats(c_in, 0, c_out) if transposed else L.fgmm_hidden_packed_floats(c_out, c_a, c_in - c_a)
    packed, Wd, bd = torch.empty(floats, device="cuda"), dv(W), None if b is None else dv(b)
    ok(L.fgmm_hidden_pack(_lib.ctx(0), None, Wd.data_ptr(), ptr(bd), c_out, c_a, c_in - c_a, int(transposed), packed.data_ptr()))
    return packed


def dgrad(W, c_a, act, gy, out, want_a=True, want_b=True, off=0):
    """-> dxa, dxb (numpy; NaN where not asked for: nothing was written)"""
    (c_out, c_in), (n, _, hw) = W.shape, gy.shape
    pt, g_d, o_d = pack(W, None, c_a, True), dv(gy, off), dv(out, off)
    da, db = (torch.full((n, c, hw), float("nan"), device="cuda") for c in (c_a, c_in - c_a))
    ok(_lib.lib().fgmm_hidden_dgrad(_lib.ctx(0), None, pt.data_ptr(), c_out, c_a, c_in - c_a, act, SLOPE, g_d.data_ptr(), o_d.data_ptr(),
                                    ptr(da) if want_a else None, ptr(db) if want_b else None, n, hw))
    return da.cpu().numpy(), db.cpu().numpy()


def wgrad(xa, xb, gy, out, act, c_a, want_w=True, want_b=True):
    (n, c_out, hw), c_b, L = gy.shape, xb.shape[1], _lib.lib()
    nbytes = L.fgmm_hidden_wgrad_workspace(c_out, c_a, c_b, int(xa is not None), n, hw)
    ws, dw, db = torch.empty(nbytes // 4, device="cuda"), torch.full((c_out, c_a + c_b), float("nan"), device="cuda"), torch.full((c_out,), float("nan"), device="cuda")
    t = [None if xa is None else dv(xa), dv(xb), dv(gy), dv(out)]
    ok(L.fgmm_hidden_wgrad(_lib.ctx(0), None, ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), c_out, c_a, c_b, act, SLOPE, n, hw, ptr(dw) if want_w else None,
                           ptr(db) if want_b else None, ws.data_ptr(), nbytes))
    return dw.cpu().numpy(), db.cpu().numpy()


@pytest.mark.parametrize("absent", [False, True])
def test_apply_packed_is_a_handle_s_apply_bit_for_bit(absent):
    c_a, c_b, c_out, hw, n = 5, 40, 33, 129, 2
    W, b, xa, xb, _, _ = make(1, c_a, c_b, c_out, hw, n)
    a_d, b_d = None if absent else dv(xa), dv(xb)
    got, want = (torch.full((n, c_out, hw), float("nan"), device="cuda") for _ in range(2))
    rc, h = create(W, b, c_a, LEAKY, SLOPE)
    ok(rc)
    ok(_lib.lib().fgmm_hidden_apply(_lib.ctx(0), None, h, ptr(a_d), b_d.data_ptr(), want.data_ptr(), n, hw))
    ok(_lib.lib().fgmm_hidden_apply_packed(_lib.ctx(0), None, pack(W, b, c_a, False).data_ptr(), c_out, c_a, c_b, LEAKY, SLOPE, ptr(a_d), b_d.data_ptr(),
                                           got.data_ptr(), n, hw))
    _lib.lib().fgmm_hidden_destroy(h)
    assert not torch.isnan(want).any() and torch.equal(got.view(torch.int32), want.view(torch.int32))


# c_a = 5, c_b = 40: a row tile straddles dxa and dxb.  ask: both | b (xa absent: dxa NULL) | a (dxb NULL alone) | off (an address off the 16-byte grid)
DGRAD = [(c_out, hw, act, "both") for c_out in (1, 33) for hw in (1, 3, 129, 260) for act in (NONE, LEAKY, RELU)] + [(33, 260, LEAKY, ask) for ask in ("b", "a", "off")]


@pytest.mark.parametrize("c_out,hw,act,ask", DGRAD)
def test_dgrad_equals_the_chain_bit_for_bit(oracle, c_out, hw, act, ask):
    c_a, c_b, n = 5, 40, 2
    W, _, _, _, gy, out = make(c_out + hw + act, c_a, c_b, c_out, hw, n)
    da, db = dgrad(W, c_a, act, gy, out, ask != "b", ask != "a", int(ask == "off"))
    gz, Wt = gz_ref(gy, out, act), np.ascontiguousarray(W.T)
    for i in range(n):
        want, got = oracle.head_params(Wt, None, gz[i]), np.concatenate([da[i], db[i]])
        rows = slice(c_a if ask == "b" else 0, c_a if ask == "a" else c_a + c_b)
        assert np.array_equal(bits(got[rows]), bits(want[rows])) and np.isnan(np.delete(got, rows, 0)).all()
        err = np.abs(want.astype(np.float64) - H.exact(Wt, None, gz[i]))
        assert (err <= (H.gamma(c_out) + c_out * 2.0**-52) * H.abs_sum(Wt, None, gz[i])).all()


def wgrad_def(oracle, x, gz):
    """x [n, c, hw], gz [n, c_out, hw] -> the definition: (dW [c_out, c] with the bias' column last, float64 sum, float64 sum of |terms|)"""
    xs, gs = (np.concatenate(list(t), 1) for t in (x, gz))  # the positions of all items, concatenated
    xs = np.concatenate([xs, np.ones((1, xs.shape[1]), F32)])
    parts = [oracle.head_params(gs[:, a:b], None, np.ascontiguousarray(xs[:, a:b].T)) for a, b in G.slice_ranges(xs.shape[1])]
    acc = parts[0]
    for p in parts[1:]:
        acc = (acc + p).astype(F32)
    return acc, gs.astype(np.float64) @ xs.T.astype(np.float64), np.abs(gs.astype(np.float64)) @ np.abs(xs.T.astype(np.float64))


# (3, 171): P = 513 - three slices of 192, both slice edges inside an item; c_b = 100: with c_a = 5 and the bias' column six column tiles
# - a second block with two idle waves.  ask: all | absent (xa NULL: its columns +0) | w | b (one output alone)
WGRAD = [(n, hw, c_out, c_b, "all") for n, hw in ((3, 171), (1, 1)) for c_out in (33, 129) for c_b in (40, 100)] + [(3, 171, 33, 40, ask) for ask in ("absent", "w", "b")]


@pytest.mark.parametrize("n,hw,c_out,c_b,ask", WGRAD)
def test_wgrad_equals_its_definition_bit_for_bit(oracle, n, hw, c_out, c_b, ask):
    c_a, act = 5, (NONE, LEAKY, RELU)[(c_out // 32 + c_b // 40 + n) % 3]
    _, _, xa, xb, gy, out = make(n + hw + c_out + c_b, c_a, c_b, c_out, hw, n)
    assert G.slices(n * hw) == ((3, 192) if n == 3 else (1, 32))
    dw, db = wgrad(None if ask == "absent" else xa, xb, gy, out, act, c_a, ask != "b", ask != "w")
    want, exact, scale = wgrad_def(oracle, xb if ask == "absent" else np.concatenate([xa, xb], 1), gz_ref(gy, out, act))
    if ask == "absent":
        assert (bits(dw[:, :c_a]) == 0).all()
        dw = dw[:, c_a:]
    assert np.isnan(dw).all() if ask == "b" else np.array_equal(bits(dw), bits(want[:, :-1]))
    assert np.isnan(db).all() if ask == "w" else np.array_equal(bits(db), bits(want[:, -1]))
    S, L = G.slices(n * hw)
    assert (np.abs(want - exact) <= (H.gamma(L + S) + n * hw * 2.0**-52) * scale).all()


def dgrad_height(n, hw, rows):
    """section 2d's rule on this device: 2c's ladder over the groups of T row tiles that hold an asked row (here: all rows)"""
    outer, cus = n * -(-hw // 128), torch.cuda.get_device_properties(0).multi_processor_count
    return next((T for T in (5, 2) if outer * -(-rows // (32 * T)) >= cus), 1)


def wgrad_height(P, n_col_tiles, c_out):
    """section 5c's rule: blocks = slices x groups of four column tiles x groups of T row tiles, wanted: 256"""
    outer = G.slices(P)[0] * -(-n_col_tiles // 4)
    return next((T for T in (4, 2) if outer * -(-(-(-c_out // 32)) // T) >= 256), 1)


# (by 2c's rule two row tiles never take T = 2 - one block of five holds them as one block of two does: T = 2 needs three or four)
@pytest.mark.parametrize("T,n,rows", [(5, 256, 160), (5, 256, 64), (2, 128, 96)])
def test_dgrad_every_block_height_gives_the_same_bits(T, n, rows):
    c_a, c_out = 5, 33
    assert dgrad_height(n, 1, rows) == T and dgrad_height(1, 1, rows) == 1
    W, _, _, _, gy, out = make(T + rows, c_a, rows - c_a, c_out, 1, n)
    da, db = dgrad(W, c_a, LEAKY, gy, out)
    for i in range(n):
        la, lb = dgrad(W, c_a, LEAKY, gy[i:i + 1], out[i:i + 1])
        assert np.array_equal(bits(la[0]), bits(da[i])) and np.array_equal(bits(lb[0]), bits(db[i])), i


@pytest.mark.parametrize("T,c_out", [(4, 512), (2, 256)])
def test_wgrad_every_block_height_gives_the_same_bits(T, c_out):
    c_a, c_b, n, hw = 5, 480, 4, 1024
    assert wgrad_height(n * hw, 1 + 15 + 1, c_out) == T and wgrad_height(n * hw, 1 + 2 + 1, 33) == 1
    _, _, xa, xb, gy, out = make(T, c_a, c_b, c_out, hw, n)
    dw, db = wgrad(xa, xb, gy, out, RELU, c_a)
    lw, lb = wgrad(xa, np.ascontiguousarray(xb[:, :35]), np.ascontiguousarray(gy[:, :33]), np.ascontiguousarray(out[:, :33]), RELU, c_a)
    assert np.array_equal(bits(dw[:33, :40]), bits(lw)) and np.array_equal(bits(db[:33]), bits(lb))


def conv64(ctx, side, W, b, act):
    z = torch.nn.functional.conv2d(side if ctx is None else torch.cat([ctx, side], 1), W[:, -side.shape[1]:, None, None] if ctx is None else W[:, :, None, None], b)
    return z if act == NONE else torch.nn.functional.leaky_relu(z, SLOPE if act == LEAKY else 0.0)


@pytest.mark.parametrize("act", [NONE, LEAKY, RELU])
@pytest.mark.parametrize("absent", [False, True])
def test_pointwise_layer_against_float64_autograd(act, absent):
    """the operator's output and four gradients against float64 autograd of conv2d + activation on cat(ctx, side), by the bounds above
    with two more roundings in each gamma: gz is formed in binary32 (gy * slope) from an output that carries the activation's own
    rounding.  Then the same bits with any subset of requires_grad, on the caller's non-default stream, and run to run."""
    c_a, c_b, c_out, h, w, n = 5, 40, 33, 3, 43, 2
    W, b, xa, xb, gy, _ = make(40 + act, c_a, c_b, c_out, h * w, n)
    leaf = lambda a, shape=None: torch.from_numpy(a).cuda().reshape(shape or a.shape).requires_grad_(True)
    t = [None if absent else leaf(xa, (n, c_a, h, w)), leaf(xb, (n, c_b, h, w)), leaf(W), leaf(b)]
    g = torch.from_numpy(gy).cuda().reshape(n, c_out, h, w)
    out = pointwise_layer(*t, ACT_NAME[act], SLOPE)
    grads = torch.autograd.grad(out, [v for v in t if v is not None], g)
    t64 = [None if v is None else v.detach().double().requires_grad_(True) for v in t]
    out64 = conv64(*t64, act)
    grads64 = torch.autograd.grad(out64, [v for v in t64 if v is not None], g.double())
    a64 = [None if v is None else v.detach().abs() for v in t64]
    gz = torch.where(out64 > 0, g.double(), g.double() * (SLOPE if act == LEAKY else 0.0)).abs() if act != NONE else g.double().abs()
    assert ((out.double() - out64).abs() <= H.gamma(c_a + c_b + 2) * conv64(a64[0], a64[1], a64[2], a64[3], NONE) + 2.0**-149).all()
    sums = torch.autograd.grad(conv64(*[None if v is None else v.requires_grad_(True) for v in a64], NONE), [v for v in a64 if v is not None], gz)  # sums of |terms|
    S, L = G.slices(n * h * w)
    names = (["ctx"] if not absent else []) + ["side", "weight", "bias"]
    for name, got, want, scale in zip(names, grads, grads64, sums):
        gam = H.gamma(c_out + 2) if name in ("ctx", "side") else H.gamma(L + S + 2)
        err = (got.double() - want).abs()
        print(f"{name}: max err {float(err.max()):.3e}, max err / bound {float((err / (gam * scale + 2.0**-149)).max()):.3f}")
        assert (err <= gam * scale + 2.0**-149).all(), name
    first = dict(zip(names, grads))
    s = torch.cuda.Stream()
    for asked in (names, ["weight"], ["side"], [names[0], "bias"]):
        for v, name in zip([v for v in t if v is not None], names):
            v.requires_grad_(name in asked)
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            again = torch.autograd.grad(pointwise_layer(*t, ACT_NAME[act], SLOPE), [v for v in t if v is not None and v.requires_grad], g)
        s.synchronize()
        assert all(torch.equal(a.view(torch.int32), first[name].view(torch.int32)) for a, name in zip(again, asked)), asked


class Wide(torch.nn.Module):
    """a float32 module's float64 copy behind casts: the un-fused codec's parameter network in float64"""

    def __init__(self, net):
        super().__init__()
        self.net = copy.deepcopy(net).double()

    def forward(self, x):
        return self.net(x.double()).float()


def test_checkerboard_forward_with_the_fused_body_and_head():
    """fused body and head (the modules silent) against the un-fused codec with a float64 parameter network.  Three layers of at most 56
    inputs, each within gamma(56) = 3.4e-6 of its sum of |w x| (a few units): parameters within 1e-4.  A likelihood's slope in one of its
    twelve parameters is at most 0.4 / sigma, sigma >= the scale bound 0.11: 12 x 3.6 x 1e-4 = 4e-3, the same relative to a gradient's largest element."""
    from tests.test_gpu_ckbd_context_grad import MaskedConv, _grads
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    M, h, w, B = 4, 6, 10, 2
    torch.manual_seed(7)
    last = torch.nn.Conv2d(40, 12 * M, 1)
    with torch.no_grad():
        last.bias[: 4 * M] += 1.0  # sigma mostly positive
    ep = torch.nn.Sequential(torch.nn.Conv2d(2 * M + 2 * M, 56, 1), torch.nn.LeakyReLU(), torch.nn.Conv2d(56, 40, 1), torch.nn.ReLU(), last)
    ctx_net = MaskedConv(M, 2 * M)
    mk = lambda e, **kw: CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, mode="polya")}, entropy_parameters=e,
                                                 context_prediction=copy.deepcopy(ctx_net), forward_method="onepass", **kw).cuda().eval()
    fused, plain = mk(copy.deepcopy(ep), fuse_body=True, fuse_head=True), mk(torch.nn.Sequential(Wide(ep)))
    calls = []
    for m in fused.entropy_parameters:
        m.register_forward_hook(lambda *_: calls.append(1))
    rng = np.random.default_rng(2)
    y = dv((rng.standard_normal((B, M, h, w)) * 4).astype(F32))
    side = dv(rng.standard_normal((B, 2 * M, h, w)).astype(F32))
    res = []
    for codec in (fused, plain):
        like = codec(y, side)["likelihoods"]["y"]
        (-torch.log2(like)).sum().backward()
        res.append((like.detach().double(), _grads(codec)))
    assert not calls and torch.isfinite(res[0][0]).all()
    assert float((res[0][0] - res[1][0]).abs().max()) <= 4e-3
    for name, g in res[0][1].items():
        ref = res[1][1][name.replace("entropy_parameters.", "entropy_parameters.0.net.")]
        rel = float((g.double() - ref.double()).abs().max() / ref.double().abs().max())
        assert rel <= 4e-3, name
