"""GPU: dense 3x3 / 5x5 convolution layers on the matrix cores (header section 5d; fgmm_conv.hip, ConvStack, HyperLatentCodec(fuse_h_s=True),
ChannelGroupsLatentCodec(fuse_channel_context=True)).  Bars: bit for bit tests/conv_ref.py's chain; the same bits from every block
height; the derived float64 bound; the ABI's refusals; the codecs' parameters those of ConvStack."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from flashgmm_amd import ConvStack, _lib
from tests import conv_ref as R
from tests import head_ref as H
from tests.test_conv_stack_cpu import h_s

pytestmark = pytest.mark.gpu
NONE, LEAKY, RELU = R.NONE, R.LEAKY, R.RELU
bits = lambda a: a.view(np.uint32)
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()


def create(W, b, act=NONE, slope=0.0, shuffle=1, k=None, c_out=None, c_in=None):
    hd, Wd, bd = C.c_void_p(), dv(W), None if b is None else dv(b)
    rc = _lib.lib().fgmm_conv_create(_lib.ctx(0), None, Wd.data_ptr(), None if b is None else bd.data_ptr(), W.shape[0] if c_out is None else c_out,
                                     W.shape[1] if c_in is None else c_in, W.shape[-1] if k is None else k, act, slope, shuffle, C.byref(hd))
    return rc, hd


def run(W, b, x, act=NONE, slope=0.0, shuffle=1, wider=0):
    """the raw ABI -> numpy; wider: x is the leading channels of a tensor with that many more, all NaN"""
    rc, hd = create(W, b, act, slope, shuffle)
    assert rc == 0, _lib.lib().fgmm_last_error()
    n, c_in, h, w = x.shape
    xd = dv(np.concatenate([x, np.full((n, wider, h, w), np.nan, R.F32)], 1))
    out = torch.full((n, W.shape[0] // shuffle**2, h * shuffle, w * shuffle), float("nan"), device="cuda")
    for rep in range(2):  # (the same bits from every launch)
        assert _lib.lib().fgmm_conv_apply(_lib.ctx(0), None, hd, xd.data_ptr(), (c_in + wider) * h * w, out.data_ptr(), n, h, w) == 0, _lib.lib().fgmm_last_error()
        got = out.cpu().numpy()
        assert rep == 0 or np.array_equal(bits(got), bits(first))
        first = got
    _lib.lib().fgmm_conv_destroy(hd)
    return got


def same_bits(got, want):
    cls = H.ieee_class(want)
    return np.array_equal(H.ieee_class(got), cls) and np.array_equal(bits(got)[cls != 3], bits(want)[cls != 3])


@pytest.mark.parametrize("case", R.CASES, ids=str)
def test_layer_equals_the_fmaf_chain_bit_for_bit(oracle, case):
    k, h, w, c_in, c_out, n, shuffle, act = case
    W, b, x = R.make(sum(case), k, h, w, c_in, c_out, n, bias=c_out != 31)
    got = run(W, b, x, act, 0.01, shuffle, wider=3 if c_in == 17 else 0)  # (the NaN channels beyond c_in are never read)
    want = R.chain(oracle, W, b, x, act, 0.01, shuffle)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.abs(got - want).max()


# every height of the ladder, by the header's rule: B(T) = n * patches * ceil(row tiles / T) >= 256
@pytest.mark.parametrize("T,k,h,w,c_in,c_out", [(4, 3, 128, 256, 2, 129), (2, 5, 64, 256, 3, 65), (1, 3, 32, 64, 9, 33)], ids=str)
def test_every_block_height_gives_the_chain_s_bits(oracle, T, k, h, w, c_in, c_out):
    height = lambda hh, ww: next((t for t in (4, 2) if -(-hh // 8) * -(-ww // 16) * -(-(-(-c_out // 32)) // t) >= 256), 1)
    assert height(h, w) == T and height(11, 19) == 1
    W, b, x = R.make(T + c_out, k, h, w, c_in, c_out, 1)
    got = run(W, b, x, LEAKY, 0.01)
    assert np.array_equal(bits(got), bits(R.chain(oracle, W, b, x, LEAKY, 0.01)))
    low = run(W, b, x[:, :, :11, :19], LEAKY, 0.01)  # the same elements from the shortest block, away from the cut's halo
    assert np.array_equal(bits(low[:, :, :11 - k // 2, :19 - k // 2]), bits(got[:, :, :11 - k // 2, :19 - k // 2]))


@pytest.mark.parametrize("k,act", [(3, NONE), (5, LEAKY), (3, RELU)])
def test_special_values_follow_the_chain(oracle, k, act):
    W, b, x = R.make(70 + k, k, 5, 6, 3, 8, 2)
    x[1] = np.abs(x[1])  # (item 1: no negative input - row 3's -0 weights give -0 products only)
    x[0, 0, 0, 0], x[0, 1, 2, 3], x[0, 2, 4, 5], x[0, 0, 1, 1], x[1, 1, 0] = np.inf, -np.inf, np.nan, -0.0, 0.0
    W[1, 2, 1, 1], W[2, 0, 0, 0], W[3], b[3], W[4], W[4, 1, k // 2, k // 2] = np.nan, np.inf, -0.0, -0.0, 0.0, -1.0  # row 2: an infinite weight, outside the image for the first rows
    got, want = run(W, b, x, act, 0.01), R.chain(oracle, W, b, x, act, 0.01)
    assert same_bits(got, want) and {0, 1, 2, 3} <= set(H.ieee_class(want).ravel()) | ({2} if act == RELU else set())
    assert np.isnan(want[1, 2, 0]).all() and np.isfinite(x[1]).all()  # inf * (+0 outside the image) is NaN: the tap takes part in the chain
    assert (np.signbit(got[1, 3]) == (act != RELU)).all() and (got[1, 3] == 0).all()  # -0 bias over zero weights stays -0 (ReLU: +0)
    alone = run(W, b, x[1:], act, 0.01)  # an item alone gives the bits it has inside a batch
    assert same_bits(alone[0], got[1])


@pytest.mark.parametrize("k,c_in", [(3, 400), (5, 130)])
def test_layer_is_within_the_derived_bound_of_float64(k, c_in):
    W, b, x = R.make(k + c_in, k, 9, 10, c_in, 16, 1)
    got = run(W, b, x, LEAKY, 0.01)[0].reshape(16, -1).astype(np.float64)
    near = nn.functional.leaky_relu(nn.functional.conv2d(dv(x), dv(W), dv(b), padding=k // 2), float(np.float32(0.01))).cpu().numpy()[0].reshape(16, -1)
    want = R.act_ref(R.exact(W, b, x[0]), LEAKY, 0.01)
    bound = R.bound(W, b, x[0]) + 2.0**-24 * np.abs(want) + 2.0**-150
    for name, v in (("library", got), ("torch", near.astype(np.float64))):
        err = np.abs(v - want)
        print(f"{name} k {k} K {c_in * k * k}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), name


def test_the_abi_refuses_what_the_header_says_and_writes_nothing():
    L, ctx = _lib.lib(), _lib.ctx(0)
    W, b, x = R.make(5, 3, 4, 4, 4, 6, 1)
    for kw in [dict(k=4), dict(k=1), dict(c_out=0), dict(c_in=0), dict(act=3), dict(act=-1), dict(slope=float("inf")), dict(slope=float("nan")),
               dict(shuffle=0), dict(shuffle=3), dict(shuffle=2)]:  # (the last: c_out = 6 is no multiple of 4)
        rc, hd = create(W, b, **kw)
        assert rc == 1 and not hd.value, kw
    rc, hd = create(W, b)
    out = torch.full((3, 6, 4, 4), float("nan"), device="cuda")
    xd, o = dv(x), out[1].data_ptr()
    for args in [(xd.data_ptr(), 64, o, -1, 4, 4), (xd.data_ptr(), 64, o, 1, -4, 4), (xd.data_ptr(), 64, o, 1, 4, -4), (None, 64, o, 1, 4, 4), (xd.data_ptr(), 64, None, 1, 4, 4),
                 (xd.data_ptr(), 63, o, 1, 4, 4), (xd.data_ptr(), 1 << 40, o, 1 << 12, 1 << 13, 1 << 13)]:  # (the last: 2^31 workgroups)
        assert L.fgmm_conv_apply(ctx, None, hd, *args) == 1 and L.fgmm_last_error(), args
    for n, h, w in [(0, 4, 4), (1, 0, 4), (1, 4, 0)]:
        assert L.fgmm_conv_apply(ctx, None, hd, xd.data_ptr(), 64, o, n, h, w) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    L.fgmm_conv_destroy(hd), L.fgmm_conv_destroy(None)


def test_apply_is_ordered_on_the_caller_s_stream():
    """the input is written on a side stream behind a delay that has not run out when the call is made: after that stream's
    synchronise the output is that of the true input"""
    net = h_s().cuda()
    op, true = ConvStack(net), torch.randn(2, 8, 5, 7, device="cuda")
    with torch.no_grad():
        want, near = op(true), net(true)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        buf = torch.full_like(true, 7.0)
        torch.cuda._sleep(20_000_000)  # (about 9 ms)
        ev = torch.cuda.Event()
        buf.copy_(true), ev.record()
        got = op(buf)
        assert not ev.query(), "the producer had completed before the call returned: the case would prove nothing"
    s.synchronize()
    assert got.shape == (2, 32, 20, 28) and torch.equal(got, want) and torch.allclose(got, near, rtol=0, atol=1e-4)


class EB:  # a stand-in entropy bottleneck with the reference's contract: z_hat = round(z), "coded" as its own bytes
    def compress(self, z):
        return [torch.round(z).cpu().numpy().tobytes()]

    def decompress(self, strings, shape):
        return torch.from_numpy(np.frombuffer(strings[0], R.F32).reshape(1, -1, *shape).copy()).cuda()


def test_hyper_codec_with_the_fused_h_s():
    from flashgmm_amd.latent_codecs import HyperLatentCodec

    net = h_s().cuda()
    codec, y = HyperLatentCodec(entropy_bottleneck=EB(), h_s=net, fuse_h_s=True), torch.randn(1, 8, 6, 9, device="cuda") * 3
    hook = net.register_forward_hook(lambda *_: pytest.fail("the torch h_s ran"))
    with torch.no_grad():
        enc = codec.compress(y)
        dec, want = codec.decompress(enc["strings"], enc["shape"]), ConvStack(net)(torch.round(y))
        assert enc["params"].shape == (1, 32, 24, 36) and torch.equal(enc["params"], dec["params"]) and torch.equal(enc["params"], want)
        hook.remove()
        assert torch.allclose(want, net(torch.round(y)), rtol=0, atol=1e-4)
        net[0].weight.mul_(1.25)  # new weights: the stack is packed again
        assert not torch.equal(codec.compress(y)["params"], want)


class Rounding(nn.Module):  # a stand-in group codec: the symbols round(y - mean), the first channels of the parameters being the mean
    def compress(self, y, params):
        sym = torch.round(y - params[:, :y.shape[1]])
        return {"strings": [sym.cpu().numpy().tobytes()], "shape": y.shape[1:], "y_hat": sym + params[:, :y.shape[1]]}

    def decompress(self, strings, shape, params):
        return {"y_hat": torch.from_numpy(np.frombuffer(strings[0], R.F32).reshape(1, *shape).copy()).cuda() + params[:, :shape[0]]}


def test_channel_groups_codec_with_the_fused_channel_context():
    from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec

    cc = nn.Sequential(nn.Conv2d(4, 12, 5, padding=2), nn.ReLU(), nn.Conv2d(12, 6, 5, padding=2)).cuda()
    codec = ChannelGroupsLatentCodec(latent_codec={"y0": Rounding(), "y1": Rounding()}, channel_context={"y1": cc}, groups=[4, 6], fuse_channel_context=True)
    cc.register_forward_hook(lambda *_: pytest.fail("the torch channel context ran"))
    y, side = torch.randn(1, 10, 9, 17, device="cuda") * 3, torch.randn(1, 6, 9, 17, device="cuda")
    with torch.no_grad():
        enc = codec.compress(y, side)
        dec = codec.decompress(enc["strings"], enc["shape"], side)
        many = codec.decompress_many([enc["strings"]], enc["shape"], [side])
        assert torch.equal(dec["y_hat"], enc["y_hat"]) and torch.equal(many[0]["y_hat"], enc["y_hat"])
        ctx = ConvStack(cc)(enc["y_hat"][:, :4].contiguous())  # group 1's parameters: the stack on the slice, then the side parameters
        assert torch.equal(enc["y_hat"][:, 4:], torch.round(y[:, 4:] - ctx) + ctx)
