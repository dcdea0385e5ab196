"""GPU: the dense layers' gradients (header section 5f; fgmm_conv_grad.hip, fgmm_conv.hip's gradient staging, ops.conv_layer, ConvStack, the codecs'
forward()).  Bars: bit for bit tests/conv_grad_ref.py's chains at every block height; the float64 bounds; the refusals; forward()'s parameters compress()'s."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

from flashgmm_amd import ConvStack, _lib
from flashgmm_amd.ops import conv_layer
from tests import conv_grad_ref as G
from tests import conv_ref as R
from tests import head_ref as H
from tests.test_conv_stack_cpu import h_s
from tests.test_gpu_conv_stack import EB, Rounding, bits, create, dv, same_bits

pytestmark = pytest.mark.gpu
NONE, LEAKY, RELU, SLOPE = R.NONE, R.LEAKY, R.RELU, 0.01
L, ptr = _lib.lib, lambda t: None if t is None else t.data_ptr()
nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")
same = lambda got, want: all(np.array_equal(bits(a), bits(b)) for a, b in zip(got, want))
shaped = lambda case, seed: np.random.default_rng(seed).standard_normal((case[5], case[4] // case[6]**2, case[1] * case[6], case[2] * case[6])).astype(R.F32)
ok = lambda rc: rc == 0 or pytest.fail(L().fgmm_last_error())


def pack(W, b, transposed):
    (c_out, c_in, k, _), Wd, bd = W.shape, dv(W), None if b is None else dv(b)
    packed = torch.empty(L().fgmm_conv_packed_floats(*((c_in, c_out) if transposed else (c_out, c_in)), k), device="cuda")
    ok(L().fgmm_conv_pack(_lib.ctx(0), None, Wd.data_ptr(), ptr(bd), c_out, c_in, k, int(transposed), packed.data_ptr()))
    return packed


def grads(W, x, gy, out, act, shuffle=1, wider=0):  # the raw ABI, twice for the same bits -> dx, dW, dbias; wider: that many more channels behind x's, all NaN
    (c_out, c_in, k, _), (n, _, h, w) = W.shape, x.shape
    xd, gd, od, pt = dv(np.concatenate([x, np.full((n, wider, h, w), np.nan, R.F32)], 1)), dv(gy), dv(out), pack(W, None, True)
    nbytes = G.slices(n, h, w)[0] * c_out * (c_in * k * k + 1) * 4
    assert nbytes == L().fgmm_conv_wgrad_workspace(c_out, c_in, k, n, h, w)
    for rep in range(2):
        dx, dw, db, ws = nan(n, c_in, h, w), nan(*W.shape), nan(c_out), nan(nbytes // 4)
        ok(L().fgmm_conv_dgrad(_lib.ctx(0), None, pt.data_ptr(), c_out, c_in, k, act, SLOPE, shuffle, gd.data_ptr(), ptr(od) if act else None, dx.data_ptr(), n, h, w))
        ok(L().fgmm_conv_wgrad(_lib.ctx(0), None, xd.data_ptr(), (c_in + wider) * h * w, gd.data_ptr(), ptr(od) if act else None, c_out, c_in, k, act, SLOPE, shuffle,
                               n, h, w, ws.data_ptr(), dw.data_ptr(), db.data_ptr()))
        got = [t.cpu().numpy() for t in (dx, dw, db)]
        assert rep == 0 or same(got, first)
        first = got
    return got


# the launchers' rules, restated.  dgrad: B(T) = n * patches * ceil(ceil(c_in / 32) / T) >= 256; wgrad: S * column groups * ceil(ceil(c_out / 32) / T) >= 256
dgrad_height = lambda k, h, w, c_in, c_out, n: next((t for t in (4, 2) if n * -(-h // 8) * -(-w // 16) * -(-(-(-c_in // 32)) // t) >= 256), 1)
wgrad_height = lambda k, h, w, c_in, c_out, n: next((t for t in (4, 2) if G.slices(n, h, w)[0] * -(-c_in // (14 if k == 3 else 10)) * -(-(-(-c_out // 32)) // t) >= 256), 1)
# (heights of dgrad, wgrad - None: the special values, which follow the chains by IEEE class, a NaN output taking gz's second branch; case).  conv_ref.CASES: the edges of the 8 x 16 patch, the chunk of 8 channels (the column groups of 14 | 10), the row tile of
# 32, the tallest block - all T = 1; (1, 9, 29): 261 positions in two bands - two slices, the second one image row; then each kernel's T = 4, 2
CASES = [((1, 1), c) for c in R.CASES + [(3, 9, 29, 15, 4, 1, 1, RELU)]] + [((4, 1), (3, 3, 2, 129, 3, 128, 1, LEAKY)), ((2, 1), (5, 3, 2, 65, 3, 128, 1, LEAKY)),
                                                                            ((1, 4), (3, 8, 32, 211, 97, 16, 1, RELU)), ((1, 2), (3, 8, 32, 99, 65, 16, 1, RELU))]


def poison(W, x, gy, out):  # -0, +-inf and NaN in every operand; item 1: x >= 0 and gy <= 0 (with ReLU and out < 0 in channel 6: +0 times positive x)
    x[1], gy[1], out[1, 6] = np.abs(x[1]), -np.abs(gy[1]), -np.abs(out[1, 6])
    x[0, 0, 0, 0], x[0, 1, 2, 3], x[0, 2, 4, 5], x[0, 0, 1, 1], x[1, 1, 0] = np.inf, -np.inf, np.nan, -0.0, 0.0
    gy[0, 1, 0, 5], gy[0, 2, 4, 0], gy[0, 3, 2, 2], gy[0, 4], gy[1, 5] = np.inf, -np.inf, np.nan, -0.0, 0.0
    out[0, 0, 1, 1], out[0, 0, 1, 2], out[0, 0, 1, 3], out[0, 1, 0, 5], out[0, 2, 4, 0], out[0, 3, 2, 2] = np.nan, np.inf, -0.0, 1.0, 1.0, 1.0  # (the last three: the special gradients pass)
    W[1, 2, 1, 1], W[2, 0, 0, 0], W[3], W[4] = np.nan, np.inf, -0.0, 0.0


@pytest.mark.parametrize("heights,case", CASES + [(None, (k, 5, 6, 3, 8, 2, 1, act)) for k, act in ((3, NONE), (5, LEAKY), (3, RELU))], ids=str)
def test_apply_packed_and_the_gradients_equal_their_chains_bit_for_bit(oracle, heights, case):
    k, h, w, c_in, c_out, n, shuffle, act = case
    W, b, x = R.make(sum(case), k, h, w, c_in, c_out, n)
    rc, hd = create(W, b, act, SLOPE, shuffle)
    xd, got, want = dv(x), *(nan(n, c_out // shuffle**2, h * shuffle, w * shuffle) for _ in range(2))
    ok(rc), ok(L().fgmm_conv_apply(_lib.ctx(0), None, hd, xd.data_ptr(), c_in * h * w, want.data_ptr(), n, h, w))
    ok(L().fgmm_conv_apply_packed(_lib.ctx(0), None, pack(W, b, False).data_ptr(), c_out, c_in, k, act, SLOPE, shuffle, xd.data_ptr(), c_in * h * w, got.data_ptr(), n, h, w))
    L().fgmm_conv_destroy(hd)
    assert not torch.isnan(want).any() and torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert heights is None or heights == (dgrad_height(*case[:6]), wgrad_height(*case[:6]))
    gy, out = shaped(case, sum(case)), shaped(case, sum(case) + 1000)
    if heights is None:
        poison(W, x, gy, out)
    g = G.gz(gy, out, act, SLOPE, shuffle)
    assert heights or act == NONE or bits(g[0, 0, 1, 1:2])[0] == bits(np.array([gy[0, 0, 1, 1] * R.F32(SLOPE) if act == LEAKY else 0], R.F32))[0]
    rows = [0, 31, 32, c_out - 1] if c_out * c_in > 5000 else slice(None)  # (a chain reads its own channel alone: the edges of a row tile and of the block)
    dx, dw, db = grads(W, x, gy, out, act, shuffle, wider=3 if c_in == 17 else 0)
    want = (G.data_grad(oracle, W, g),) + G.weight_grad(oracle, x, g, k, rows)
    assert all((same_bits if heights is None else lambda a, b: np.array_equal(bits(a), bits(b)))(a, b) for a, b in zip((dx, dw[rows], db[rows]), want))
    assert heights or {0, 3} < set(H.ieee_class(want[0]).ravel()) and {0, 3} <= set(H.ieee_class(want[1]).ravel())  # finite, NaN and an infinity


@pytest.mark.parametrize("k,c_in,c_out", [(3, 40, 130), (5, 130, 16)])
def test_gradients_are_within_the_derived_bound_of_float64(k, c_in, c_out):  # (no activation: gz is gy exactly; the kernels AND torch's own backward)
    (W, _, x), gy = R.make(k + c_in, k, 9, 17, c_in, c_out, 2), shaped((k, 9, 17, c_in, c_out, 2, 1), k)
    t = [dv(v).requires_grad_(True) for v in (x, W, np.zeros(c_out, R.F32))]
    near = [v.cpu().numpy() for v in torch.autograd.grad(nn.functional.conv2d(*t, padding=k // 2), t, dv(gy))]
    for name, got in (("library", grads(W, x, gy, gy, NONE)), ("torch", near)):
        assert all((np.abs(v.astype(np.float64) - want) <= bound).all() for v, want, bound in zip(got, *G.exact(x, W, gy))), name


@pytest.mark.parametrize("case", [(3, 9, 17, 9, 36, 2, 2, LEAKY), (5, 5, 6, 11, 8, 1, 1, RELU)], ids=str)
def test_conv_layer_gives_the_abi_s_bits_for_every_subset_asked(case):
    """on the leading channels of a wider tensor (the others NaN): the raw calls' bits, +0 in dx of the channels not read; then on a side stream behind a delayed input"""
    k, h, w, c_in, c_out, n, shuffle, act = case
    W, b, x = R.make(sum(case), k, h, w, c_in, c_out, n)
    gy, t = shaped(case, 1), [dv(np.concatenate([x, np.full((n, 2, h, w), np.nan, R.F32)], 1)), dv(W), dv(b)]
    fwd = lambda: conv_layer(*t, {LEAKY: "leaky_relu", RELU: "relu"}[act], SLOPE, shuffle, channels=c_in)
    run = lambda asked, g: torch.autograd.grad(fwd(), [t[i] for i in asked], g)
    cut = lambda asked, got: [(v[:, :c_in] if i == 0 else v).cpu().numpy() for i, v in zip(asked, got)]
    want = grads(W, x, gy, fwd().cpu().numpy(), act, shuffle)
    for asked in ([0, 1, 2], [0], [1], [2], [0, 2], [1, 2]):
        for i, v in enumerate(t):
            v.requires_grad_(i in asked)
        got = run(asked, dv(gy))
        assert same(cut(asked, got), [want[i] for i in asked]) and (0 not in asked or (bits(got[0][:, c_in:].cpu().numpy()) == 0).all()), asked
    s, true, gd = torch.cuda.Stream(), t[0].detach().clone(), dv(gy)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t[0] = torch.full_like(true, 7.0).requires_grad_(True)
        torch.cuda._sleep(20_000_000)  # (about 9 ms)
        ev = torch.cuda.Event()
        t[0].data.copy_(true), ev.record()
        late = run([0, 1, 2], gd)
        assert not ev.query(), "the producer had completed before the calls returned: the case would prove nothing"
    s.synchronize()
    assert same(cut([0, 1, 2], late), want)


def test_the_abi_refuses_what_the_header_says_and_writes_nothing():
    buf, pk, ctx = nan(4096), torch.zeros(L().fgmm_conv_packed_floats(8, 4, 3) + 1, device="cuda"), _lib.ctx(0)
    base = dict(c_out=8, c_in=4, k=3, act=LEAKY, slope=SLOPE, shuffle=1, n=1, h=4, w=4, p=pk.data_ptr(), x=buf[1024:].data_ptr(), gy=buf[2048:].data_ptr(), out=buf[3072:].data_ptr(),
                o=buf.data_ptr(), ws=buf[512:].data_ptr(), stride=64, bias=None, tr=1)
    calls = {"d": (L().fgmm_conv_dgrad, "p c_out c_in k act slope shuffle gy out o n h w"), "w": (L().fgmm_conv_wgrad, "x stride gy out c_out c_in k act slope shuffle n h w ws o bias"),
             "a": (L().fgmm_conv_apply_packed, "p c_out c_in k act slope shuffle x stride o n h w"), "p": (L().fgmm_conv_pack, "x bias c_out c_in k tr p")}
    bad = [("dwap", dict(k=4)), ("dwap", dict(c_out=0)), ("dwap", dict(c_in=0)), ("dwa", dict(act=3)), ("dwa", dict(slope=float("nan"))), ("dw", dict(slope=-0.5)), ("dwa", dict(shuffle=3)),
           ("dwa", dict(shuffle=2, c_out=6)), ("dwa", dict(n=-1)), ("dwa", dict(h=-1)), ("dw", dict(gy=None)), ("dw", dict(out=None)), ("dwa", dict(o=None)), ("dap", dict(p=base["p"] + 4)),
           ("dap", dict(p=None)), ("wap", dict(x=None)), ("w", dict(ws=None)), ("w", dict(ws=base["ws"] + 4)), ("wa", dict(stride=63)), ("p", dict(bias=base["gy"])), ("p", dict(tr=2))]
    for which, kw in bad:
        for fn, names in (calls[c] for c in which):
            assert fn(ctx, None, *({**base, **kw}[a] for a in names.split())) == 1 and L().fgmm_last_error(), (fn.__name__, kw)
    assert L().fgmm_conv_dgrad(ctx, None, *({**base, "n": 0}[a] for a in calls["d"][1].split())) == 0 and L().fgmm_conv_packed_floats(8, 4, 4) == 0  # nothing to do: no launch
    torch.cuda.synchronize()
    assert torch.isnan(buf).all() and (pk == 0).all()


def test_conv_stack_under_autograd_against_float64():
    """the handles' bits in the forward; every gradient within gamma(D) of the float64 sum of |terms|: D = 2 sum over the layers of (c_in k^2 + 2) roundings
    forward and back, the sum the same gradient of the stack with |weights| on |x|, |g|.  First order: a branch flip within rounding of zero is not in it"""
    net, x = h_s().cuda(), torch.randn(2, 8, 5, 7, device="cuda", requires_grad=True)
    stack, hook = ConvStack(net), net.register_forward_hook(lambda *_: pytest.fail("the torch stack ran"))
    out = stack(x)
    g = torch.randn_like(out)
    got = torch.autograd.grad(out, [x] + list(net.parameters()), g)
    with torch.no_grad():
        assert torch.equal(out, stack(x.detach()))
    hook.remove()
    net64, mag, x64 = copy.deepcopy(net).double(), copy.deepcopy(net).double(), x.detach().double()
    with torch.no_grad():
        [p.abs_() for p in mag.parameters()]
    want, scale = (torch.autograd.grad(m(v), [v] + list(m.parameters()), gg) for m, v, gg in ((net64, x64.requires_grad_(True), g.double()), (mag, x64.abs().requires_grad_(True), g.double().abs())))
    D = 2 * sum(m.in_channels * 9 + 2 for m in net.modules() if isinstance(m, nn.Conv2d))
    for a, c, s in zip(got, want, scale):
        assert a.shape == c.shape and ((a.double() - c).abs() <= H.gamma(D) * s + 2.0**-149).all()
    for kw in (dict(arithmetic="bf16x6"), dict(transposed=True)):
        with pytest.raises(RuntimeError, match=next(iter(kw))):
            ConvStack(net, **kw)(x)


def test_the_codecs_forward_reports_the_parameters_compress_codes_with():
    from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec, HyperLatentCodec

    EBF = type("EBF", (EB,), {"__call__": lambda self, z: (torch.round(z), torch.ones_like(z))})  # forward()'s half of the stand-ins' contracts; y_hat as compress gives it
    RoundingF = type("RoundingF", (Rounding,), {"forward": lambda self, y, p: {"likelihoods": {"y": torch.ones_like(y)}, "y_hat": torch.round(y - p[:, :y.shape[1]]) + p[:, :y.shape[1]]}})
    net, cc = h_s().cuda(), nn.Sequential(nn.Conv2d(4, 12, 5, padding=2), nn.ReLU(), nn.Conv2d(12, 6, 5, padding=2)).cuda()
    for m in (net, cc):
        m.register_forward_hook(lambda *_: pytest.fail("the torch module ran"))
    hyper, y = HyperLatentCodec(entropy_bottleneck=EBF(), h_s=net, fuse_h_s=True), torch.randn(1, 8, 6, 9, device="cuda") * 3
    params = hyper(y)["params"]
    params.square().sum().backward()
    groups = ChannelGroupsLatentCodec(latent_codec={"y0": RoundingF(), "y1": RoundingF()}, channel_context={"y1": cc}, groups=[4, 6], fuse_channel_context=True)
    yg, side = torch.randn(1, 10, 9, 17, device="cuda") * 3, torch.randn(1, 6, 9, 17, device="cuda")
    y_hat = groups(yg, side)["y_hat"]
    y_hat.sum().backward()  # (round has no gradient: what arrives is the context's own)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for m in (net, cc) for p in m.parameters())
    with torch.no_grad():  # the point of the feature: the same bits as the coder's
        assert torch.equal(params, hyper.compress(y)["params"]) and torch.equal(params, hyper(y)["params"]) and torch.equal(y_hat, groups.compress(yg, side)["y_hat"])
