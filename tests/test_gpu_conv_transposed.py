"""GPU: transposed 3x3 / 5x5 convolution layers of stride 1 | 2 on the matrix cores (header section 5e; fgmm_deconv.hip, the flipped pack of
fgmm_conv.hip, ConvStack(transposed=True), HyperLatentCodec(fuse_h_s="transposed")).  Bars: bit for bit tests/deconv_ref.py's chain; the
same bits from every launch form; special values; the derived float64 bound; the ABI's refusals; the codec's parameters those of ConvStack."""
import ctypes as C

import numpy as np
import pytest
import torch
from torch import nn

from flashgmm_amd import ConvStack, _lib
from tests import deconv_ref as D
from tests import head_ref as H
from tests.test_conv_transposed_cpu import elic_h_s
from tests.test_gpu_conv_stack import EB, bits, dv, same_bits

pytestmark = pytest.mark.gpu
NONE, LEAKY, RELU = D.NONE, D.LEAKY, D.RELU


def create(W, b, s, act=NONE, slope=0.0, k=None, c_in=None, c_out=None):
    hd, Wd, bd = C.c_void_p(), dv(W), None if b is None else dv(b)
    rc = _lib.lib().fgmm_conv_create_transposed(_lib.ctx(0), None, Wd.data_ptr(), None if b is None else bd.data_ptr(), W.shape[0] if c_in is None else c_in,
                                                W.shape[1] if c_out is None else c_out, W.shape[-1] if k is None else k, s, act, slope, C.byref(hd))
    return rc, hd


def run(W, b, x, s, act=NONE, slope=0.0, wider=0):
    """the raw ABI -> numpy; wider: x is the leading channels of a tensor with that many more, all NaN"""
    rc, hd = create(W, b, s, act, slope)
    assert rc == 0, _lib.lib().fgmm_last_error()
    n, c_in, h, w = x.shape
    xd = dv(np.concatenate([x, np.full((n, wider, h, w), np.nan, D.F32)], 1))
    out = torch.full((n, W.shape[1], s * h, s * w), float("nan"), device="cuda")
    for rep in range(2):  # (the same bits from every launch)
        assert _lib.lib().fgmm_conv_apply(_lib.ctx(0), None, hd, xd.data_ptr(), (c_in + wider) * h * w, out.data_ptr(), n, h, w) == 0, _lib.lib().fgmm_last_error()
        got = out.cpu().numpy()
        assert rep == 0 or np.array_equal(bits(got), bits(first))
        first = got
    _lib.lib().fgmm_conv_destroy(hd)
    return got


@pytest.mark.parametrize("case", D.CASES, ids=str)
def test_layer_equals_the_fmaf_chain_bit_for_bit(oracle, case):
    k, s, h, w, c_in, c_out, n, act = case
    W, b, x = D.make(sum(case), k, h, w, c_in, c_out, n, bias=(h, w) != (3, 5))
    got = run(W, b, x, s, act, 0.01, wider=3 if (h, w) == (3, 5) else 0)  # (the NaN channels beyond c_in are never read)
    want = D.chain(oracle, W, b, x, s, act, 0.01)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.abs(got - want).max()


# every launch form, by the header's rule: 1 if P ceil(R / 2) >= 256, else 2 if P R >= 256, else 3; P = n patches, R = ceil(c_out / 32)
@pytest.mark.parametrize("form,k,h,w,c_in,c_out", [(1, 5, 128, 256, 2, 33), (2, 3, 64, 256, 3, 33), (3, 5, 32, 64, 3, 33)], ids=str)
def test_every_launch_form_gives_the_chain_s_bits(oracle, form, k, h, w, c_in, c_out):
    rule = lambda hh, ww: (lambda P, Rt: 1 if P * -(-Rt // 2) >= 256 else 2 if P * Rt >= 256 else 3)(-(-hh // 8) * -(-ww // 16), -(-c_out // 32))
    assert rule(h, w) == form and rule(11, 19) == 3
    W, b, x = D.make(form + c_out, k, h, w, c_in, c_out, 1)
    got = run(W, b, x, 2, LEAKY, 0.01)
    assert np.array_equal(bits(got), bits(D.chain(oracle, W, b, x, 2, LEAKY, 0.01)))
    low = run(W, b, x[:, :, :11, :19], 2, LEAKY, 0.01)  # the same elements from the last form, away from the cut (an output reads up to row r + 1)
    assert np.array_equal(bits(low[:, :, :20, :36]), bits(got[:, :, :20, :36]))


@pytest.mark.parametrize("k,act", [(5, NONE), (3, LEAKY), (5, RELU)])
def test_special_values_follow_the_chain(oracle, k, act):
    W, b, x = D.make(90 + k, k, 5, 6, 3, 8, 2)
    x[1] = np.abs(x[1])  # (item 1: no negative input - channel 3's -0 weights give -0 products only)
    x[0, 0, 0, 0], x[0, 1, 2, 3], x[0, 2, 4, 5], x[0, 0, 1, 1], x[1, 1, 0] = np.inf, -np.inf, np.nan, -0.0, 0.0
    W[0, 0], W[2, 1, 1, 1], W[0, 2, 0, 0], W[:, 3], b[3] = np.abs(W[0, 0]), np.nan, np.inf, -0.0, -0.0  # W[0, 2, 0, 0]: the tap (k - 1, k - 1), input (r + 1, q + 1)
    got, want = run(W, b, x, 2, act, 0.01), D.chain(oracle, W, b, x, 2, act, 0.01)
    assert same_bits(got, want) and {0, 1, 2, 3} <= set(H.ieee_class(want).ravel()) | ({2} if act == RELU else set())
    # an infinite input leaves finite every output without a term on it: x[0, 0, 0, 0] and (k = 5) out[2 r + 1][2 q + 1] at (r - 1, q) =
    # (0, 0), (k = 3) out[2 r][2 q] at (r - 1, q - 1) = (0, 0) - a zero-padded 3x3 over the input grid multiplies a planted 0 by it
    assert np.isfinite(got[0, 0, 3, 1] if k == 5 else got[0, 0, 2, 2]) and np.isinf(got[0, 0, 0, 0])
    # inf weight * (+0 outside the image) is NaN: the tap (k - 1, k - 1) belongs to phase (0, 0) for k = 5, (1, 1) for k = 3, and reads
    # row h of a finite item for that phase's last row
    par = int(k == 3)
    assert np.isnan(got[1, 2, 8 + par, par::2]).all() and not np.isnan(got[1, 2, 2 + par, par:10:2]).any() and np.isfinite(x[1]).all()
    assert (np.signbit(got[1, 3]) == (act != RELU)).all() and (got[1, 3] == 0).all()  # -0 bias over -0 weights stays -0 (ReLU: +0)
    alone = run(W, b, x[1:], 2, act, 0.01)  # an item alone gives the bits it has inside a batch
    assert same_bits(alone[0], got[1])


def test_layer_is_within_the_derived_bound_of_float64():
    W, b, x = D.make(135, 5, 9, 10, 130, 16, 1)
    got = run(W, b, x, 2, LEAKY, 0.01)[0].astype(np.float64)
    near = nn.functional.leaky_relu(nn.functional.conv_transpose2d(dv(x), dv(W), dv(b), stride=2, padding=2, output_padding=1), float(np.float32(0.01))).cpu().numpy()[0]
    want = D.act_ref(D.exact(W, b, x[0], 2), LEAKY, 0.01)
    bound = D.bound(W, b, x[0], 2) + 2.0**-24 * np.abs(want) + 2.0**-150
    for name, v in (("library", got), ("torch", near.astype(np.float64))):
        err = np.abs(v - want)
        print(f"{name} k 5 s 2 c_in 130: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert (np.abs(got - want) <= bound).all()


def test_the_abi_refuses_what_the_header_says_and_writes_nothing():
    L, ctx = _lib.lib(), _lib.ctx(0)
    W, b, x = D.make(5, 3, 4, 4, 4, 6, 1)
    for s, kw in [(0, {}), (3, {}), (-1, {}), (2, dict(k=4)), (1, dict(k=1)), (2, dict(c_out=0)), (2, dict(c_in=0)), (2, dict(act=3)), (1, dict(act=-1)),
                  (2, dict(slope=float("inf"))), (2, dict(slope=float("nan")))]:
        rc, hd = create(W, b, s, **kw)
        assert rc == 1 and not hd.value and L.fgmm_last_error(), (s, kw)
    xd = dv(x)
    for s in (1, 2):
        rc, hd = create(W, b, s)
        out = torch.full((3, 6, 4 * s, 4 * s), float("nan"), device="cuda")
        o = out[1].data_ptr()
        for args in [(xd.data_ptr(), 64, o, -1, 4, 4), (xd.data_ptr(), 64, o, 1, -4, 4), (xd.data_ptr(), 64, o, 1, 4, -4), (None, 64, o, 1, 4, 4),
                     (xd.data_ptr(), 64, None, 1, 4, 4), (xd.data_ptr(), 63, o, 1, 4, 4), (xd.data_ptr(), 1 << 40, o, 1, 1 << 15, 1 << 15)]:  # (the last: 2^30 positions)
            assert L.fgmm_conv_apply(ctx, None, hd, *args) == 1 and L.fgmm_last_error(), args
        assert L.fgmm_conv_apply(ctx, None, None, xd.data_ptr(), 64, o, 1, 4, 4) == 1
        for n, h, w in [(0, 4, 4), (1, 0, 4), (1, 4, 0)]:
            assert L.fgmm_conv_apply(ctx, None, hd, xd.data_ptr(), 64, o, n, h, w) == 0
        torch.cuda.synchronize()
        assert torch.isnan(out).all()
        L.fgmm_conv_destroy(hd)


def test_hyper_codec_with_the_fused_transposed_h_s():
    from flashgmm_amd.latent_codecs import HyperLatentCodec

    net = elic_h_s(8).cuda()
    codec, y = HyperLatentCodec(entropy_bottleneck=EB(), h_s=net, fuse_h_s="transposed"), torch.randn(1, 8, 6, 9, device="cuda") * 3
    hook = net.register_forward_hook(lambda *_: pytest.fail("the torch h_s ran"))
    with torch.no_grad():
        enc = codec.compress(y)
        dec, want = codec.decompress(enc["strings"], enc["shape"]), ConvStack(net, transposed=True)(torch.round(y))
        assert enc["params"].shape == (1, 16, 24, 36) and torch.equal(enc["params"], dec["params"]) and torch.equal(enc["params"], want)
        hook.remove()
        assert torch.allclose(want, net(torch.round(y)), rtol=0, atol=1e-4)
        net[0].weight.mul_(1.25)  # new weights: the stack is packed again
        assert not torch.equal(codec.compress(y)["params"], want)
