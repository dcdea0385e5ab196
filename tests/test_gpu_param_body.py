"""GPU: the parameter network's hidden layers on the matrix cores (header section 2c; fgmm_hidden.hip, ParameterBody, CheckerboardLatentCodec(
fuse_body=True)).  Bars: bit for bit oracle.head_params' fmaf chain over cat(xa, xb) - over xb alone for an absent xa - then the activation
restated below; the same bits from every block height; the derived float64 bound; the codec's strings those of a codec calling ParameterBody."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import ParameterBody, _lib
from tests import head_ref as H

pytestmark = pytest.mark.gpu
F32 = np.float32
NONE, LEAKY, RELU = _lib.FGMM_ACT_NONE, _lib.FGMM_ACT_LEAKY, _lib.FGMM_ACT_RELU


def act_ref(v, act, slope):
    with np.errstate(all="ignore"):
        if act == LEAKY:
            return np.where(v > 0, v, v * v.dtype.type(F32(slope)))  # (the layer's slope is the binary32 number)
        return np.where(v > 0, v, np.where(np.isnan(v), v, np.zeros_like(v))) if act == RELU else v


def dv(a, off=0):
    """numpy -> device tensor; off: its address moved by that many floats (off the 16-byte grid)"""
    t = torch.empty(a.size + off, dtype=torch.float32, device="cuda")[off:].view(a.shape)
    return t.copy_(torch.from_numpy(np.ascontiguousarray(a)))


def create(W, b, c_a, act=NONE, slope=0.0, c_out=None):
    h = C.c_void_p()
    Wd, bd = dv(W), None if b is None else dv(b)
    rc = _lib.lib().fgmm_hidden_create(_lib.ctx(0), None, Wd.data_ptr(), None if b is None else bd.data_ptr(), W.shape[0] if c_out is None else c_out, c_a,
                                       W.shape[1] - c_a, act, slope, C.byref(h))
    return rc, h


def run(W, b, xa, xb, act=NONE, slope=0.0, c_a=None, off=0):
    """the raw ABI: W [c_out, c_a + c_b], xa [n, c_a, hw] or None (absent when c_a > 0), xb [n, c_b, hw] -> out [n, c_out, hw] (numpy)"""
    c_a = (0 if xa is None else xa.shape[1]) if c_a is None else c_a
    rc, h = create(W, b, c_a, act, slope)
    assert rc == 0, _lib.lib().fgmm_last_error()
    n, _, hw = xb.shape
    a_d, b_d = None if xa is None else dv(xa, off), dv(xb, off)
    out = torch.full((n, W.shape[0], hw), float("nan"), device="cuda")
    for _ in range(2):  # (the same bits from every launch)
        rc = _lib.lib().fgmm_hidden_apply(_lib.ctx(0), None, h, None if xa is None else a_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), n, hw)
        assert rc == 0, _lib.lib().fgmm_last_error()
        got = out.cpu().numpy()
        assert _ == 0 or np.array_equal(got.view(np.uint32), first.view(np.uint32))
        first = got
    _lib.lib().fgmm_hidden_destroy(h)
    return got


def chain(oracle, W, b, xa, xb, act, slope, c_a):
    x, Wc = (xb, W[:, c_a:]) if xa is None else (np.concatenate([xa, xb], 1), W)
    return np.stack([act_ref(oracle.head_params(Wc, b, xi), act, slope) for xi in x])


def same_bits(got, want):
    cls = H.ieee_class(want)
    return np.array_equal(H.ieee_class(got), cls) and np.array_equal(got.view(np.uint32)[cls != 3], want.view(np.uint32)[cls != 3])


def make(seed, c_a, c_b, c_out, hw, n, bias=True):
    r = np.random.default_rng(seed)
    g = lambda *s: r.standard_normal(s).astype(F32)
    return g(c_out, c_a + c_b), g(c_out) if bias else None, g(n, c_a, hw) if c_a else None, g(n, c_b, hw)


def height(n, hw, c_out):
    """the header's rule, on this device"""
    outer, n_rt, cus = n * -(-hw // 128), -(-c_out // 32), torch.cuda.get_device_properties(0).multi_processor_count
    return next((T for T in (5, 2) if outer * -(-n_rt // T) >= cus), 1)


# (c_a, c_b, c_out, hw, n, act, bias, absent, off): sources not a multiple of the K tile, one tile plus one, a single source; c_out 1, 33 and
# around the tallest block's 160 rows; positions 1, 3 (element loads), 127 | 128 | 129 (the position tile's edge), 260 (16-byte loads)
CASES = [(0, 1, 1, 1, 1, NONE, True, False, 0), (1, 31, 33, 3, 3, LEAKY, True, False, 0), (33, 31, 159, 127, 1, RELU, False, False, 0),
         (32, 65, 160, 128, 1, LEAKY, True, False, 0), (40, 33, 161, 129, 3, NONE, True, False, 0), (33, 31, 33, 260, 1, LEAKY, True, False, 0),
         (32, 65, 1, 260, 3, RELU, True, False, 1), (40, 33, 33, 128, 1, LEAKY, True, True, 0), (1, 31, 160, 3, 1, RELU, True, True, 0),
         (33, 31, 161, 260, 1, NONE, False, True, 1), (0, 1, 33, 127, 3, RELU, True, False, 0), (0, 33, 159, 129, 1, LEAKY, False, False, 0),
         (32, 65, 33, 1, 1, NONE, True, True, 0), (0, 33, 160, 260, 3, NONE, True, False, 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_b%d_o%d_hw%d_n%d_act%d_b%d_abs%d_off%d" % c)
def test_layer_equals_the_fmaf_chain_bit_for_bit(oracle, case):
    c_a, c_b, c_out, hw, n, act, bias, absent, off = case
    W, b, xa, xb = make(sum(case), c_a, c_b, c_out, hw, n, bias)
    xa = None if absent else xa
    got = run(W, b, xa, xb, act, 0.01, c_a, off)
    want = chain(oracle, W, b, xa, xb, act, 0.01, c_a)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.abs(got - want).max()
    assert (got < 0).any() or act == RELU or c_out * hw * n < 4  # (the activation's negative side is exercised)


# every height of the ladder, by the header's rule on 256 compute units; c_in <= 40 keeps the oracle quick
@pytest.mark.parametrize("T,c_a,c_b,c_out,hw", [(5, 8, 8, 33, 32768), (5, 4, 4, 161, 16384), (2, 4, 4, 96, 16384), (1, 20, 20, 161, 260)],
                         ids=lambda v: str(v))
def test_every_block_height_gives_the_chain_s_bits(oracle, T, c_a, c_b, c_out, hw):
    assert height(1, hw, c_out) == T and height(1, 260, c_out) == 1
    W, b, xa, xb = make(T + c_out, c_a, c_b, c_out, hw, 1)
    got = run(W, b, xa, xb, LEAKY, 0.01)
    assert np.array_equal(got.view(np.uint32), chain(oracle, W, b, xa, xb, LEAKY, 0.01, c_a).view(np.uint32))
    low = run(W, b, xa[:, :, :260], xb[:, :, :260], LEAKY, 0.01)  # the same elements from the shortest block
    assert np.array_equal(low.view(np.uint32), got[:, :, :260].view(np.uint32))


@pytest.mark.parametrize("act", [NONE, LEAKY, RELU])
def test_special_values_follow_the_chain_and_the_absent_source_differs_where_the_header_says(oracle, act):
    c_a, c_b, c_out, hw = 3, 5, 8, 16
    W, b, xa, xb = make(77, c_a, c_b, c_out, hw, 1)
    xb[0, :, 0], xb[0, 1, 1], xb[0, 2, 2], xb[0, 3, 3], xb[0, 0, 4] = -0.0, np.inf, -np.inf, np.nan, 0.0
    W[1, 4], W[2, 5], W[3], b[3], W[4], W[4, 4] = np.inf, np.nan, 0.0, -0.0, 0.0, -1.0  # row 3: -0 bias over zero weights; row 4: -x[1]
    for a in (xa, None):
        got, want = run(W, b, a, xb, act, 0.01, c_a), chain(oracle, W, b, a, xb, act, 0.01, c_a)
        assert same_bits(got, want)
        assert {0, 1, 2, 3} <= set(H.ieee_class(want).ravel()) or act == RELU
    pre = chain(oracle, W, b, None, xb, NONE, 0.0, c_a)[0]  # the pre-activations the three activations met: -0, -inf and NaN among them
    assert np.signbit(pre[3, 0]) and pre[3, 0] == 0 and pre[4, 1] == -np.inf and np.isnan(pre[2]).all()
    # absent against explicit zeros: equal for finite weights and random biases ...
    Wf, bf = make(78, c_a, c_b, c_out, hw, 1)[:2]
    zeros = np.zeros_like(xa)
    assert np.array_equal(run(Wf, bf, None, xb, act, 0.01, c_a).view(np.uint32)[:, :, 5:], run(Wf, bf, zeros, xb, act, 0.01, c_a).view(np.uint32)[:, :, 5:])
    # ... a non-finite weight of the absent columns makes NaN of explicit zeros only; a chain at -0 stays -0 in the absent form only
    Wf[5, 1] = np.inf
    bf[6], Wf[6] = -0.0, 0.0
    ab, ex = run(Wf, bf, None, xb, act, 0.01, c_a)[0], run(Wf, bf, zeros, xb, act, 0.01, c_a)[0]
    assert np.isfinite(ab[5, 5:]).all() and np.isnan(ex[5]).all()
    assert ab[6, 0] == 0 and ex[6, 0] == 0 and np.signbit(ab[6, 0]) == (act != RELU) and not np.signbit(ex[6, 0])


@pytest.mark.parametrize("c_a,c_b,c_out,hw,act,slope", [(48, 48, 80, 96, LEAKY, 0.01), (0, 80, 80, 96, LEAKY, 0.01), (384, 384, 16, 20, RELU, 0.0), (384, 384, 16, 20, LEAKY, -2.5)])
def test_layer_is_within_the_derived_bound_of_float64(c_a, c_b, c_out, hw, act, slope):
    """the chain's error through an activation of Lipschitz constant max(1, |slope|), and the one rounding of LeakyReLU's multiply"""
    W, b, xa, xb = make(c_a + c_out, c_a, c_b, c_out, hw, 2)
    got = run(W, b, xa, xb, act, slope)
    for i in range(2):
        x = xb[i] if xa is None else np.concatenate([xa[i], xb[i]])
        want = act_ref(H.exact(W, b, x), act, slope)
        bound = max(1.0, abs(slope)) * H.chain_bound(W, b, x) + 2.0**-24 * np.abs(want) + 2.0**-150
        err = np.abs(got[i].astype(np.float64) - want)
        print(f"c_in {c_a + c_b}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert (err <= bound).all()


def test_the_abi_refuses_what_the_header_says_and_writes_nothing():
    L, ctx = _lib.lib(), _lib.ctx(0)
    W, b, xa, xb = make(5, 4, 4, 8, 16, 1)
    for kw, c_a in [(dict(act=3), 4), (dict(act=-1), 4), (dict(slope=float("inf")), 4), (dict(slope=float("nan")), 4), ({}, -1), ({}, 8)]:
        rc, h = create(W, b, c_a, **kw)  # (c_a = 8 leaves c_b = 0)
        assert rc == 1 and not h.value, (kw, c_a)
    assert create(W, b, 4, c_out=0)[0] == 1
    (_, two), (_, one) = create(W, b, 4), create(W, b, 0)
    out = torch.full((3, 8, 16), float("nan"), device="cuda")
    a_d, b_d, o = dv(xa), dv(xb), out[1].data_ptr()
    for h, args in [(two, (a_d.data_ptr(), None, o, 1, 16)), (two, (a_d.data_ptr(), b_d.data_ptr(), None, 1, 16)), (two, (None, b_d.data_ptr(), o, -1, 16)),
                    (two, (None, b_d.data_ptr(), o, 1, -1)), (one, (a_d.data_ptr(), b_d.data_ptr(), o, 1, 16)), (two, (None, b_d.data_ptr(), o, 1 << 10, 1 << 30))]:  # (the last: 2^33 workgroups)
        assert L.fgmm_hidden_apply(ctx, None, h, *args) == 1 and L.fgmm_last_error(), args
    for n, hw in [(0, 16), (1, 0)]:
        assert L.fgmm_hidden_apply(ctx, None, two, a_d.data_ptr(), b_d.data_ptr(), o, n, hw) == 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    L.fgmm_hidden_destroy(two), L.fgmm_hidden_destroy(one), L.fgmm_hidden_destroy(None)


def test_apply_is_ordered_on_the_caller_s_stream():
    """the sources are written on a side stream behind a delay that has not run out when the call is made: after that stream's
    synchronise the output is that of the true sources"""
    body = torch.nn.Sequential(torch.nn.Conv2d(40, 33, 1), torch.nn.LeakyReLU(0.2), torch.nn.Conv2d(33, 9, 1)).cuda()
    op = ParameterBody(body, 8)
    true = [torch.randn(2, 8, 5, 7, device="cuda"), torch.randn(2, 32, 5, 7, device="cuda")]
    with torch.no_grad():
        want, near = op.features(*true), body(torch.cat(true, 1))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        bufs = [torch.full_like(t, 7.0) for t in true]
        torch.cuda._sleep(20_000_000)  # (about 9 ms)
        ev = torch.cuda.Event()
        bufs[0].copy_(true[0]), bufs[1].copy_(true[1]), ev.record()
        got = op.features(*bufs)
        assert not ev.query(), "the producer had completed before the call returned: the case would prove nothing"
    s.synchronize()
    assert got.shape == (2, 9, 5, 7) and torch.equal(got, want) and torch.allclose(got, near, rtol=0, atol=1e-4)


class BodyModule(torch.nn.Module):  # entropy_parameters[:-1] calling ParameterBody itself on the merged tensor (the anchors' context: explicit zeros)
    def __init__(self, mods, c_ctx):
        super().__init__()
        self.mods, self.c_ctx = mods, c_ctx

    def forward(self, x):
        return ParameterBody(self.mods, self.c_ctx).features(x[:, :self.c_ctx], x[:, self.c_ctx:])


@pytest.mark.parametrize("fuse_head,fuse_context,act", [(False, False, "leaky"), (True, False, "leaky"), (True, True, "leaky"), (False, True, "relu")])
def test_checkerboard_codec_with_the_fused_body(fuse_head, fuse_context, act):
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec
    from tests import ckbd_ctx_ref as R

    M, h, w = 32, 16, 24
    torch.manual_seed(3)
    ctx_net, last, A = torch.nn.Conv2d(M, 2 * M, 5, padding=2), torch.nn.Conv2d(80, 12 * M, 1), torch.nn.LeakyReLU if act == "leaky" else torch.nn.ReLU
    with torch.no_grad():
        ctx_net.weight.copy_(torch.from_numpy(R.masked(ctx_net.weight.numpy())))
        last.bias[: 4 * M] += 1.0  # sigma mostly positive
    ep, ctx_net = torch.nn.Sequential(torch.nn.Conv2d(4 * M, 96, 1), A(), torch.nn.Conv2d(96, 80, 1), A(), last).cuda(), ctx_net.cuda()
    gmm = lambda: GaussianMixtureConditionalLatentCodec(K=4)
    fused = CheckerboardLatentCodec(latent_codec={"y": gmm()}, entropy_parameters=ep, context_prediction=ctx_net, fuse_head=fuse_head, fuse_context=fuse_context, fuse_body=True)
    plain = CheckerboardLatentCodec(latent_codec={"y": gmm()}, entropy_parameters=torch.nn.Sequential(BodyModule(ep[:-1], 2 * M), ep[-1]), context_prediction=ctx_net,
                                    fuse_head=fuse_head, fuse_context=fuse_context)
    calls, outs, rng = [], [], np.random.default_rng(9)
    for m in ep[:-1]:
        m.register_forward_hook(lambda *_: calls.append(1))
    with torch.no_grad():
        for img in range(2):
            y = torch.from_numpy((rng.standard_normal((1, M, h, w)) * 4).astype(F32)).cuda()
            side = torch.from_numpy(rng.standard_normal((1, 2 * M, h, w)).astype(F32)).cuda()
            a, b = fused.compress(y, side), plain.compress(y, side)
            assert a["shape"] == b["shape"] and torch.equal(a["y_hat"], b["y_hat"]) and torch.equal(a["y_hat"], torch.round(y))
            for (sa, ama, za), (sb, amb, zb_) in zip(a["strings"], b["strings"]):
                assert bytes(sa) == bytes(sb) and ama == amb and torch.equal(za.cpu(), zb_.cpu())
            assert torch.equal(fused.decompress(a["strings"], a["shape"], side)["y_hat"], a["y_hat"])
            outs.append((a, side))
        many = fused.decompress_many([o[0]["strings"] for o in outs], outs[0][0]["shape"], [o[1] for o in outs])
        assert all(torch.equal(m_["y_hat"], a["y_hat"]) for m_, (a, _) in zip(many, outs))
        assert not calls  # the torch body never ran
        ep[2].weight.mul_(1.25)  # new weights in a hidden layer: the body is packed again
        c = fused.compress(y, side)
        assert any(bytes(x[0]) != bytes(z[0]) for x, z in zip(c["strings"], a["strings"]))
        assert torch.equal(fused.decompress(c["strings"], c["shape"], side)["y_hat"], c["y_hat"]) and not calls
