"""GPU (-m gpu): the checkerboard context convolution on the matrix cores (include/flashgmm_amd.h section 5b,
flashgmm_amd/csrc/fgmm_ckbd_ctx.hip; flashgmm_amd.ops.CheckerboardContext; CheckerboardLatentCodec(fuse_context=True)).

Bars: the operator is BIT FOR BIT tests/ckbd_ctx_ref.chain - the oracle's fmaf chain over the 12 kept taps, row-major, and the input
channels of each, from the bias - at every shape of the corpus under both parities, with -0, infinities and NaN among the features
(NaN compared by class), for a filter of zeros with a -0 bias, item by item of a batch, and run to run; torch's own path on the GPU is
held by head_ref.chain_bound against float64 (its gap to the kernel is printed, not asserted tighter); the C ABI refuses what the
header says it refuses and writes nothing; the call is ordered on the caller's stream; a codec with fuse_context round-trips."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from flashgmm_amd.ops import CheckerboardContext
from tests import ckbd_ctx_ref as R
from tests import head_ref as H
from tests.test_gpu_streams import delay, pending, streams  # noqa: F401  (the fixtures and THE helper of the stream tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class MaskedConv(torch.nn.Conv2d):
    """the stand-in for the reference's CheckerboardMaskedConv2d (compressai/layers): a 5x5 convolution whose weight is multiplied by
    a mask buffer that keeps the kernel positions (i, j) with i + j odd"""

    def __init__(self, c_in, c_out, bias=True):
        super().__init__(c_in, c_out, 5, padding=2, bias=bias)
        self.register_buffer("mask", torch.from_numpy(R.masked(np.ones((c_out, c_in, 5, 5), np.float32))))

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.weight * self.mask, self.bias, padding=2)


class NeverRun(MaskedConv):
    def forward(self, x):
        raise AssertionError("the context convolution ran as a torch module")


def module_of(W, b, cls=MaskedConv):
    """W need not be masked: the module's mask buffer does it"""
    conv = cls(W.shape[1], W.shape[0], bias=b is not None)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(W))
        if b is not None:
            conv.bias.copy_(torch.from_numpy(b))
    return conv.to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_is_the_chain(got, W, b, A, parity):
    """got [N, C_out, h, w/2] (numpy) against the chain, item by item: NaN by class, everything else by bit pattern"""
    for n in range(A.shape[0]):
        want = R.chain(W, b, A[n], parity)
        cg, cw = H.ieee_class(got[n]), H.ieee_class(want)
        assert np.array_equal(cg, cw), (n, int((cg != cw).sum()))
        same = (bits(got[n]) == bits(want)) | (cw == 3)
        assert same.all(), (n, int((~same).sum()), np.abs(got[n] - want)[~same].max())


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("case", R.CORPUS, ids=lambda c: "h%d_w%d_M%d_C%d_N%d" % c)
def test_the_operator_is_the_chain_bit_for_bit(case, parity):
    h, w, M, C_out, N = case
    W, b, A = R.make_case(200 + h + M, h, w, M, C_out, N)
    op = CheckerboardContext(module_of(W, b), parity)
    assert (op.M, op.C_out, op.anchor_parity) == (M, C_out, parity)
    got = op.non_anchor(dv(A))
    assert got.shape == (N, C_out, h, w // 2) and got.dtype == torch.float32
    assert_is_the_chain(got.cpu().numpy(), W, b, A, parity)
    # item k of a batch is the same item alone; two consecutive calls are equal
    again = op.non_anchor(dv(A))
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    for k in range(N):
        alone = op.non_anchor(dv(A[k:k + 1]))
        assert torch.equal(alone[0].view(torch.int32), got[k].view(torch.int32)), k


def _row_tiles_per_block(n, h, w, c_out):
    """the launcher's rule (fgmm_ckbd_ctx.hip, ckbd_ctx_tiles), restated: the most row tiles of 32 output channels per block - 6, 2 or 1 -
    at which n items of ceil(h w/2 / 128) position tiles still make 256 blocks; 1 when none does"""
    pt, n_rt = -(-(h * (w // 2)) // 128), -(-c_out // 32)
    return next((T for T in (6, 2) if n * pt * -(-n_rt // T) >= 256), 1)


# (h, w, M, C_out, N, row tiles per block): the kernel's three instantiations where the launcher itself picks them, and its threshold
# from both sides.  Few channels: the oracle's chain stays cheap at these many positions.
PATHS = [
    (128, 512, 1, 1, 1, 6),   # 256 position tiles: exactly 256 blocks of six row tiles (five of them padding)
    (64, 256, 2, 193, 2, 6),  # 2 items x 64 position tiles x 2 row groups: the second group holds one real row tile, one real row in it
    (100, 256, 2, 193, 1, 2),  # 100 x 2 groups of six < 256 <= 100 x 4 groups of two: the last group half padding
    (255, 256, 1, 1, 1, 1),   # 255 blocks at six and at two: one row tile per block, far past the corpus' sizes
]


@pytest.mark.parametrize("case", PATHS, ids=lambda c: "h%d_w%d_M%d_C%d_N%d_T%d" % c)
def test_every_instantiation_is_the_chain_where_the_launcher_picks_it(case):
    h, w, M, C_out, N, T = case
    assert _row_tiles_per_block(N, h, w, C_out) == T
    assert all(_row_tiles_per_block(c[4], c[0], c[1], c[3]) == 1 for c in R.CORPUS)  # (the corpus runs the smallest block throughout)
    W, b, A = R.make_case(300 + h, h, w, M, C_out, N)
    got = CheckerboardContext(module_of(W, b), "odd").non_anchor(dv(A))
    assert_is_the_chain(got.cpu().numpy(), W, b, A, "odd")


@pytest.mark.parametrize("parity", R.PARITIES)
def test_without_a_bias_and_with_raw_weights_behind_a_mask(parity):
    """no bias: the chain starts at +0; the module's weight has non-zero dropped taps, its mask buffer removes them"""
    h, w, M, C_out, N = 5, 6, 33, 33, 1
    rng = np.random.default_rng(31)
    W = rng.standard_normal((C_out, M, 5, 5)).astype(np.float32)
    A = R.make_case(32, h, w, M, C_out, N)[2]
    got = CheckerboardContext(module_of(W, None), parity).non_anchor(dv(A))
    assert_is_the_chain(got.cpu().numpy(), R.masked(W), None, A, parity)
    plain = torch.nn.Conv2d(M, C_out, 5, padding=2).to(DEV)  # no mask buffer, dropped taps not zero: refused
    with pytest.raises(ValueError):
        CheckerboardContext(plain, parity)


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("shape", [(5, 6, 33, 33, 3), (9, 30, 2, 31, 1)])
def test_signed_zeros_infinities_and_nan_among_the_features(shape, parity):
    h, w, M, C_out, N = shape
    W, b, A = R.make_case(41, h, w, M, C_out, N)
    rng = np.random.default_rng(42)
    flat = A.reshape(-1)
    planted = [-0.0, np.inf, -np.inf, np.nan, -0.0, np.inf]
    where = rng.choice(flat.size, len(planted), replace=False)
    flat[where] = planted
    A[0, :, 0, 0] = -0.0  # a corner whose every channel is -0
    want_cls = np.concatenate([H.ieee_class(R.chain(W, b, A[n], parity)).reshape(-1) for n in range(N)])
    assert {0, 3} <= set(want_cls.tolist()) and ({1, 2} & set(want_cls.tolist()))  # the case holds what it plants
    got = CheckerboardContext(module_of(W, b), parity).non_anchor(dv(A))
    assert_is_the_chain(got.cpu().numpy(), W, b, A, parity)


@pytest.mark.parametrize("parity", R.PARITIES)
def test_a_filter_of_zeros_with_a_minus_zero_bias_comes_out_as_the_chain_says(parity):
    """acc = -0; fmaf(+0, x, acc): the product is -0 for a negative or -0 feature and +0 otherwise, and -0 + +0 = +0 - so the filter is
    -0 exactly where every tap lies inside the image over negative features, +0 elsewhere.  The kernel's padding (weights +0, features
    -0) must leave either alone."""
    h, w, M, C_out = 5, 6, 33, 33
    W, b, A = R.make_case(51, h, w, M, C_out, 1)
    A = -np.abs(A) - 1  # every feature negative
    W[7] = 0.0
    b[7] = -0.0
    want = R.chain(W, b, A[0], parity)[7]
    assert (bits(want) == 0x80000000).any() and (bits(want) == 0).any() and (want == 0).all()
    got = CheckerboardContext(module_of(W, b), parity).non_anchor(dv(A)).cpu().numpy()
    assert np.array_equal(bits(got[0, 7]), bits(want))
    assert_is_the_chain(got, W, b, A, parity)


def _torch_path_gpu(conv, A, parity):
    """unembed(conv(embed([A, 0])))[1] with the library's own data movement, the convolution torch's (MIOpen)"""
    from flashgmm_amd.ops import ckbd_embed, ckbd_unembed

    with torch.no_grad():
        return ckbd_unembed(conv(ckbd_embed(torch.stack([A, torch.zeros_like(A)]), parity)), parity)[1]


@pytest.mark.parametrize("parity", R.PARITIES)
def test_the_torch_path_is_within_the_chain_bound_of_float64(parity, capsys):
    h, w, M, C_out, N = 9, 30, 65, 193, 1
    W, b, A = R.make_case(61, h, w, M, C_out, N)
    conv = module_of(W, b)
    ref = _torch_path_gpu(conv, dv(A), parity).cpu().numpy()
    got = CheckerboardContext(conv, parity).non_anchor(dv(A)).cpu().numpy()
    exact, bound = R.exact(W, b, A[0], parity), R.bound(W, b, A[0], parity)
    err_t, err_k = np.abs(ref[0] - exact), np.abs(got[0] - exact)
    with capsys.disabled():
        print(f"\n[ckbd context {parity}] |torch - f64| max {err_t.max():.3e} ({(err_t / bound).max():.3f} of the bound), "
              f"|kernel - f64| max {err_k.max():.3e} ({(err_k / bound).max():.3f}), |torch - kernel| max {np.abs(ref - got).max():.3e}")
    assert (err_t <= bound).all(), (err_t / bound).max()
    assert (err_k <= bound).all(), (err_k / bound).max()


def test_the_c_abi_refuses_and_writes_nothing():
    h, w, M, C_out, n = 3, 4, 2, 3, 2
    W, b, A = R.make_case(71, h, w, M, C_out, n)
    op = CheckerboardContext(module_of(W, b), "even")
    L, ctx = _lib.lib(), _lib.ctx(0)
    a = dv(A)
    guard, body = 64, n * C_out * h * (w // 2)
    pattern = 0x7FC12345  # a NaN
    buf = torch.full((guard + body + guard,), pattern, dtype=torch.int32, device=DEV)
    out = buf.data_ptr() + 4 * guard
    torch.cuda.synchronize()

    def call(anchors=a.data_ptr(), out_=out, n_=n, h_=h, w_=w, odd=0, handle=op._h):
        return L.fgmm_ckbd_ctx_apply(ctx, None, handle, anchors, out_, n_, h_, w_, odd)

    refused = [dict(w_=5), dict(w_=0), dict(w_=-2), dict(h_=0), dict(n_=-1), dict(anchors=None), dict(out_=None), dict(odd=2), dict(handle=None),
               dict(h_=1 << 31, w_=4), dict(h_=1 << 24, w_=1 << 9), dict(h_=1 << 22, w_=1 << 9, n_=1 << 20)]
    for kw in refused:
        assert call(**kw) == 1, kw  # FGMM_ERR_INVALID
        assert b"context convolution" in L.fgmm_last_error()
    torch.cuda.synchronize()
    assert bool((buf == pattern).all())
    # n == 0 succeeds, with or without tensors, and launches nothing
    assert call(n_=0) == 0 and call(n_=0, anchors=None, out_=None) == 0
    torch.cuda.synchronize()
    assert bool((buf == pattern).all())
    # ... and the accepted call writes its n * C_out * h * w/2 outputs between the guards, nothing else
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((buf[:guard] == pattern).all()) and bool((buf[guard + body:] == pattern).all())
    got = buf[guard:guard + body].view(torch.float32).reshape(n, C_out, h, w // 2).cpu().numpy()
    assert_is_the_chain(got, W, b, A, "even")
    # create: a dropped tap that is not +-0 is refused by the library itself; -0 is accepted
    out_h = C.c_void_p()
    Wb = W.copy()
    Wb[1, 1, 4, 4] = 1e-40  # (a subnormal is not zero)
    wd = dv(Wb)
    assert L.fgmm_ckbd_ctx_create(ctx, None, wd.data_ptr(), None, M, C_out, C.byref(out_h)) == 1 and not out_h.value
    Wz = W.copy()
    Wz[1, 1, 4, 4] = -0.0
    wd = dv(Wz)
    assert L.fgmm_ckbd_ctx_create(ctx, None, wd.data_ptr(), None, M, C_out, C.byref(out_h)) == 0 and out_h.value
    L.fgmm_ckbd_ctx_destroy(out_h)
    L.fgmm_ckbd_ctx_destroy(None)


def test_the_call_is_ordered_on_the_callers_stream(streams, delay):  # noqa: F811
    """stream-ordered like the calls of section 5: the anchors' producer is still pending on the caller's stream when the call is made,
    the result is consumed by work enqueued on that stream afterwards, and by another stream behind an event"""
    s1, s2, _ = streams
    h, w, M, C_out = 5, 6, 32, 33
    W, b, A = R.make_case(81, h, w, M, C_out, 1)
    A_d = R.make_case(82, h, w, M, C_out, 1)[2]
    op = CheckerboardContext(module_of(W, b), "odd")
    want = dv(R.chain(W, b, A[0], "odd"))[None]
    assert not torch.equal(want, dv(R.chain(W, b, A_d[0], "odd"))[None])
    with pending(s1, delay, [dv(A)], [dv(A_d)]) as (ab,):
        got = op.non_anchor(ab)
        twice = got + got  # enqueued after the call, on the same stream
        done = torch.cuda.Event()
        done.record()
        assert torch.equal(got, want) and torch.equal(twice, want + want)
        with torch.cuda.stream(s2):
            s2.wait_event(done)
            g2 = got.clone()
        s2.synchronize()
    assert torch.equal(g2, want)


def _codec(M, seed, ctx_cls=MaskedConv, **kw):
    """a small checkerboard codec as tests/test_gpu_head.py builds it, its context model a masked 5x5 convolution"""
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    torch.manual_seed(seed)
    ctx_net = ctx_cls(M, 2 * M).to(DEV)
    last = torch.nn.Conv2d(96, 12 * M, 1)
    with torch.no_grad():
        last.bias[: 4 * M] += 1.0  # sigma mostly positive
    ep = torch.nn.Sequential(torch.nn.Conv2d(4 * M, 96, 1), torch.nn.LeakyReLU(), last).to(DEV)
    return CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, mode="polya")}, entropy_parameters=ep,
                                   context_prediction=ctx_net, **kw)


def _latent(M, h, w, seed):
    rng = np.random.default_rng(seed)
    return dv((rng.standard_normal((1, M, h, w)) * 4).astype(np.float32)), dv(rng.standard_normal((1, 2 * M, h, w)).astype(np.float32))


@pytest.mark.parametrize("fuse_head", [False, True])
def test_a_codec_with_the_fused_context_round_trips(fuse_head):
    """compress -> decompress gives y_hat back exactly, alone and with fuse_head; the context model's forward never runs (it raises)"""
    M, h, w = 24, 10, 14
    codec = _codec(M, 5, NeverRun, fuse_context=True, fuse_head=fuse_head)
    y, side = _latent(M, h, w, 6)
    with torch.no_grad():
        a = codec.compress(y, side)
        assert len(a["strings"]) == 2 and torch.equal(a["y_hat"], torch.round(y))
        assert torch.equal(codec.decompress(a["strings"], a["shape"], side)["y_hat"], a["y_hat"])
        many = codec.decompress_many([a["strings"], a["strings"]], a["shape"], [side, side])
        assert all(torch.equal(m["y_hat"], a["y_hat"]) for m in many)
        # the non-anchors' stream depends on the context: other weights in the context model, other bytes (and the packing is refreshed)
        codec.context_prediction.weight.mul_(1.5)
        c = codec.compress(y, side)
        assert bytes(c["strings"][0][0]) == bytes(a["strings"][0][0]) and bytes(c["strings"][1][0]) != bytes(a["strings"][1][0])
        assert torch.equal(codec.decompress(c["strings"], c["shape"], side)["y_hat"], c["y_hat"])


def test_the_codec_s_contexts_are_the_operator_s_and_zeros():
    M, h, w = 24, 10, 14
    codec = _codec(M, 7, NeverRun, fuse_context=True, anchor_parity="odd")
    y_hat_ = torch.round(torch.randn((2, 1, M, h, w // 2), device=DEV) * 3)
    z = codec._ctx(y_hat_, 0)
    assert z.shape == (1, 2 * M, h, w // 2) and z.dtype == y_hat_.dtype and not bool(z.any())
    want = CheckerboardContext(codec.context_prediction, "odd").non_anchor(y_hat_[0])
    got = codec._ctx(y_hat_, 1)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # ... which is the un-fused codec's context within the chain's bound (same networks, the convolution torch's)
    plain = _codec(M, 7, MaskedConv, anchor_parity="odd")
    ref = plain._ctx(torch.stack([y_hat_[0], torch.zeros_like(y_hat_[0])]), 1)
    Wn = (plain.context_prediction.weight * plain.context_prediction.mask).detach().cpu().numpy()
    bn = plain.context_prediction.bias.detach().cpu().numpy()
    bound = R.bound(Wn, bn, y_hat_[0, 0].cpu().numpy(), "odd")
    assert (np.abs(ref[0].detach().cpu().numpy().astype(np.float64) - got[0].cpu().numpy()) <= 2 * bound).all()


def test_the_switch_off_is_the_codec_without_the_argument():
    M, h, w = 24, 10, 14
    off, none = _codec(M, 9, fuse_context=False), _codec(M, 9)
    y, side = _latent(M, h, w, 10)
    with torch.no_grad():
        a, b = off.compress(y, side), none.compress(y, side)
    assert [bytes(s[0]) for s in a["strings"]] == [bytes(s[0]) for s in b["strings"]] and torch.equal(a["y_hat"], b["y_hat"])
    assert off.fuse_context is False and none.fuse_context is False and none._context is None
