"""GPU (-m gpu): the gradients of the checkerboard context convolution (include/flashgmm_amd.h section 5c,
flashgmm_amd/csrc/fgmm_ckbd_ctx_grad.hip; flashgmm_amd.ops.checkerboard_context; the three codecs' forward()).

Bars: the weight and bias gradients are BIT FOR BIT tests/ckbd_ctx_grad_ref.weight_grad - per slice the oracle's fmaf chain over the
positions, then binary32 adds of the slices, +0 at the dropped taps - and the data gradient bit for bit ckbd_ctx_grad_ref.data_grad, on
the whole corpus under both parities, with -0, infinities and NaN among g and A (NaN compared by class), from every instantiation where
the launcher picks it, and run to run; all three lie within head_ref.gamma(L + S) x the sum of the absolute terms of float64 (each term
passes through at most L + S - 1 roundings), a bound torch's own backward on the GPU is held to as well; only what needs_input_grad
asks for is computed; the C ABI refuses what the header says it refuses and writes nothing; the calls are ordered on the caller's
stream; ckbd_unembed / ckbd_embed are differentiable; the codecs' forward() is the composition of its parts."""
import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from flashgmm_amd.ops import checkerboard_context, ckbd_embed, ckbd_unembed
from tests import ckbd_ctx_grad_ref as G
from tests import ckbd_ctx_ref as R
from tests import head_ref as H
from tests.test_gpu_streams import delay, pending, streams  # noqa: F401  (the fixtures and THE helper of the stream tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = dict(ids=lambda c: "h%d_w%d_M%d_C%d_N%d" % c[:5])
PATTERN = 0x7FC12345  # a NaN


def dv(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(DEV)  # (a copy: the shared references are read-only)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(got, want, what=""):
    """NaN by class, everything else by bit pattern"""
    cg, cw = H.ieee_class(got), H.ieee_class(want)
    assert got.shape == want.shape and np.array_equal(cg, cw), (what, int((cg != cw).sum()))
    same = (bits(got) == bits(want)) | (cw == 3)
    assert same.all(), (what, int((~same).sum()), np.abs(got - want)[~same].max())


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def wgrad_abi(A, g, parity, want_w=True, want_b=True):
    """fgmm_ckbd_ctx_wgrad on device tensors A [N, M, h, w/2], g [N, C_out, h, w/2], on the current stream -> (dW or None, dbias or None)"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    (N, M, h, w2), C_out = A.shape, g.shape[1]
    nbytes = L.fgmm_ckbd_ctx_wgrad_workspace(M, C_out, N, h, 2 * w2)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=DEV)
    dw = torch.empty((C_out, M, 5, 5), dtype=torch.float32, device=DEV) if want_w else None
    db = torch.empty((C_out,), dtype=torch.float32, device=DEV) if want_b else None
    rc = L.fgmm_ckbd_ctx_wgrad(ctx, stream(), A.data_ptr(), g.data_ptr(), M, C_out, N, h, 2 * w2, int(parity == "odd"),
                               dw.data_ptr() if want_w else None, db.data_ptr() if want_b else None, ws.data_ptr(), nbytes)
    _lib.check(rc, "wgrad")
    return dw, db


def dgrad_abi(W, g, parity):
    """the data gradient through the C ABI: the transposed pack, then apply_packed with the sizes exchanged and the other parity"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    (C_out, M), (N, _, h, w2) = W.shape[:2], g.shape
    packed = torch.empty((L.fgmm_ckbd_ctx_packed_floats(C_out, M),), dtype=torch.float32, device=DEV)
    _lib.check(L.fgmm_ckbd_ctx_pack(ctx, stream(), W.data_ptr(), None, M, C_out, 1, packed.data_ptr()), "pack")
    out = torch.empty((N, M, h, w2), dtype=torch.float32, device=DEV)
    _lib.check(L.fgmm_ckbd_ctx_apply_packed(ctx, stream(), packed.data_ptr(), C_out, M, g.data_ptr(), out.data_ptr(), N, h, 2 * w2,
                                            int(parity == "odd") ^ 1), "apply_packed")
    return out


def op_grads(W, b, A, g, parity, needs=(True, True, True)):
    """forward + backward of the operator under autograd -> (out, dA, dW, db), None where not asked for"""
    At, Wt = dv(A).requires_grad_(needs[0]), dv(W).requires_grad_(needs[1])
    bt = None if b is None else dv(b).requires_grad_(needs[2])
    out = checkerboard_context(At, Wt, bt, parity)
    out.backward(dv(g))
    return out.detach(), At.grad, Wt.grad, None if bt is None else bt.grad


_REF = {}


def reference(case, parity):
    """the definitions on the case's data, computed once and shared: -> (W, b, A, g, dA [N, M, h, w/2], dW, db)"""
    key = (case, parity)
    if key not in _REF:
        h, w, M, C_out, N = case
        W, b, A, g = G.make_case(500 + h + M + C_out, h, w, M, C_out, N)
        dW, db = G.weight_grad(A, g, parity)
        dA = np.stack([G.data_grad(W, g[n], parity) for n in range(N)])
        for a in (W, b, A, g, dA, dW, db):
            a.setflags(write=False)
        _REF[key] = (W, b, A, g, dA, dW, db)
    return _REF[key]


DROPPED = np.ones((5, 5), bool)
for _i, _j in R.TAPS:
    DROPPED[_i, _j] = False


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("case", G.CORPUS, **IDS)
def test_the_three_gradients_are_their_definitions_bit_for_bit(case, parity):
    W, b, A, g, dA, dW, db = reference(case, parity)
    out, gA, gW, gb = op_grads(W, b, A, g, parity)
    for n in range(A.shape[0]):  # (the forward is section 5b's chain)
        assert_same(out[n].cpu().numpy(), R.chain(W, b, A[n], parity), "forward")
    assert_same(gW.cpu().numpy(), dW, "dW")
    assert (bits(gW.cpu().numpy())[:, :, DROPPED] == 0).all()  # +0, not -0, at every dropped tap
    assert_same(gb.cpu().numpy(), db, "dbias")
    assert_same(gA.cpu().numpy(), dA, "dA")
    # run to run: the same bits, through the operator and through the C ABI
    _, gA2, gW2, gb2 = op_grads(W, b, A, g, parity)
    w3, b3 = wgrad_abi(dv(A), dv(g), parity)
    a3 = dgrad_abi(dv(W), dv(g), parity)
    for x, y, z in ((gA, gA2, a3), (gW, gW2, w3), (gb, gb2, b3)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))


def _row_tiles_per_block(P, M, C_out, want_w=True, want_b=True):
    """the launcher's rule (fgmm_ckbd_ctx_grad.hip, ckbd_wgrad_tiles), restated: a block is T row tiles of 32 output channels x 4 column
    tiles (12 ceil(M / 32) of the weights', one of the bias') x one slice; the most T of 4, 2 at which the launch still has 256 blocks, else 1"""
    S = G.slices(P)[0]
    n_col = (12 * -(-M // 32) if want_w else 0) + (1 if want_b else 0)
    return next((T for T in (4, 2) if S * -(-n_col // 4) * -(-(-(-C_out // 32)) // T) >= 256), 1)


# (h, w, M, C_out, N, row tiles per block): 16 slices x 4 column groups throughout; 13 row tiles in 4 groups of four (the last holds one,
# 6 of its 32 rows real) = 256 blocks; 8 row tiles: 128 blocks at four, 256 at two (the last tile 26 rows); 6 row tiles: 192 at two
PATHS = [(16, 32, 2, 390, 17, 4), (16, 32, 2, 250, 17, 2), (16, 32, 2, 190, 17, 1)]


@pytest.mark.parametrize("case", PATHS, ids=lambda c: "h%d_w%d_M%d_C%d_N%d_T%d" % c)
def test_every_instantiation_is_the_definition_where_the_launcher_picks_it(case):
    h, w, M, C_out, N, T = case
    assert _row_tiles_per_block(N * h * (w // 2), M, C_out) == T
    assert all(_row_tiles_per_block(c[4] * c[0] * (c[1] // 2), c[2], c[3]) == 1 for c in G.CORPUS)  # (the corpus runs the smallest block)
    W, b, A, g, _, dW, db = reference(case[:5], "odd")
    gw, gb = wgrad_abi(dv(A), dv(g), "odd")
    assert_same(gw.cpu().numpy(), dW, "dW")
    assert_same(gb.cpu().numpy(), db, "dbias")


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("case", [(9, 30, 2, 3, 3), (5, 6, 33, 33, 3)], **IDS)
def test_signed_zeros_infinities_and_nan_among_g_and_the_anchors(case, parity):
    h, w, M, C_out, N = case
    W, b, A, g = G.make_case(41, h, w, M, C_out, N)
    rng = np.random.default_rng(42)
    planted = [-0.0, np.inf, -np.inf, np.nan, -0.0, np.inf]
    for arr in (A, g):
        flat = arr.reshape(-1)
        flat[rng.choice(flat.size, len(planted), replace=False)] = planted
    A[0, :, 0, 0] = -0.0  # a corner whose every channel is -0
    g[0, 0] = -0.0        # an output channel whose gradient is -0 throughout one item
    dW, db = G.weight_grad(A, g, parity)
    dA = np.stack([G.data_grad(W, g[n], parity) for n in range(N)])
    cls = set(H.ieee_class(dW).reshape(-1).tolist())
    assert {0, 3} <= cls and ({1, 2} & cls)  # the case holds what it plants
    _, gA, gW, gb = op_grads(W, b, A, g, parity)
    assert_same(gW.cpu().numpy(), dW, "dW")
    assert (bits(gW.cpu().numpy())[:, :, DROPPED] == 0).all()
    assert_same(gb.cpu().numpy(), db, "dbias")
    assert_same(gA.cpu().numpy(), dA, "dA")


def unembed_slices(y, parity):
    """the reference's slicing form (checkerboard.py:333-354) in torch indexing: [n, c, h, w] -> [2, n, c, h, w/2]"""
    h, w = y.shape[-2:]
    r = torch.arange(h, device=y.device)[:, None].expand(h, w // 2)
    a, n = (torch.from_numpy(f(h, w, parity)).to(y.device) for f in (R.anchor_cols, R.non_anchor_cols))
    return torch.stack([y[..., r, a], y[..., r, n]])


def embed_slices(y_, parity):
    h, w2 = y_.shape[-2:]
    r = torch.arange(h, device=y_.device)[:, None].expand(h, w2)
    a, n = (torch.from_numpy(f(h, 2 * w2, parity)).to(y_.device) for f in (R.anchor_cols, R.non_anchor_cols))
    y = y_.new_zeros(tuple(y_.shape[1:-1]) + (2 * w2,))
    y[..., r, a] = y_[0]
    y[..., r, n] = y_[1]
    return y


@pytest.mark.parametrize("parity", R.PARITIES)
def test_the_bound_against_float64_holds_for_the_kernels_and_for_torch(parity, capsys):
    """each term of a weight gradient passes through at most L + S - 1 roundings: the three gradients lie within gamma(L + S) x the sum
    of the absolute terms of the float64 result; torch's own backward of embed -> conv2d(W * mask) -> unembed is held to the same"""
    case = (9, 30, 65, 33, 3)
    W, b, A, g, dA, dW, db = reference(case, parity)
    h, w, M, C_out, N = case
    S, L = G.slices(N * h * (w // 2))
    (ew, eb), (aw, ab) = G.weight_grad_exact(A, g, parity), G.weight_grad_abs(A, g, parity)
    ea = np.stack([G.data_grad_exact(W, g[n], parity) for n in range(N)])
    aa = np.stack([G.data_grad_abs(W, g[n], parity) for n in range(N)])
    _, gA, gW, gb = op_grads(W, b, A, g, parity)
    # torch's path (MIOpen picks the order), over the slicing form of the two permutations
    At, Wt, bt = dv(A).requires_grad_(True), dv(W).requires_grad_(True), dv(b).requires_grad_(True)
    mask = dv(R.masked(np.ones_like(W)))
    noise = torch.randn_like(At)
    y = torch.nn.functional.conv2d(embed_slices(torch.stack([At, noise]), parity), Wt * mask, bt, padding=2)
    unembed_slices(y, parity)[1].backward(dv(g))
    gam = H.gamma(L + S)
    with capsys.disabled():
        print()
        for name, k, t, e, a in (("dA", gA, At.grad, ea, aa), ("dW", gW, Wt.grad, ew, aw), ("dbias", gb, bt.grad, eb, ab)):
            k, t = k.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
            keep = a > 0
            rk, rt = (np.abs(k - e)[keep] / (gam * a[keep])).max(), (np.abs(t - e)[keep] / (gam * a[keep])).max()
            print(f"[ckbd context grad {parity}] {name}: |kernel - f64| {rk:.4f} of the bound, |torch - f64| {rt:.4f}, "
                  f"|torch - kernel| max {np.abs(t - k).max():.3e}")
    for name, k, t, e, a in (("dA", gA, At.grad, ea, aa), ("dW", gW, Wt.grad, ew, aw), ("dbias", gb, bt.grad, eb, ab)):
        k, t = k.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
        assert (np.abs(k - e) <= gam * a).all(), name
        if name == "dW":  # torch differentiates through W * mask: exact zeros at the dropped taps, like the kernel
            assert (t[:, :, DROPPED] == 0).all()
        assert (np.abs(t - e) <= gam * a).all(), name


def test_only_what_needs_input_grad_asks_for_is_computed():
    case, parity = (9, 30, 2, 3, 3), "even"
    W, b, A, g, dA, dW, db = reference(case, parity)
    _, gA, gW, gb = op_grads(W, b, A, g, parity, needs=(True, False, False))
    assert gW is None and gb is None
    assert_same(gA.cpu().numpy(), dA, "dA alone")
    _, gA, gW, gb = op_grads(W, b, A, g, parity, needs=(False, True, False))
    assert gA is None and gb is None
    assert_same(gW.cpu().numpy(), dW, "dW alone")
    _, gA, gW, gb = op_grads(W, b, A, g, parity, needs=(False, False, True))
    assert gA is None and gW is None
    assert_same(gb.cpu().numpy(), db, "dbias alone")
    _, gA, gW, gb = op_grads(W, None, A, g, parity)  # no bias: the forward's chain starts at +0, the gradients are the same
    assert gb is None
    assert_same(gW.cpu().numpy(), dW, "dW without a bias")
    assert_same(gA.cpu().numpy(), dA, "dA without a bias")
    # at the ABI: an output that is not asked for is not written - its buffer keeps the pattern it was filled with
    L, ctx = _lib.lib(), _lib.ctx(0)
    h, w, M, C_out, N = case
    Ad, gd = dv(A), dv(g)
    nbytes = L.fgmm_ckbd_ctx_wgrad_workspace(M, C_out, N, h, w)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=DEV)
    for want_w, want_b in ((True, False), (False, True)):
        bw = torch.full((C_out * M * 25,), PATTERN, dtype=torch.int32, device=DEV)
        bb = torch.full((C_out,), PATTERN, dtype=torch.int32, device=DEV)
        assert L.fgmm_ckbd_ctx_wgrad(ctx, None, Ad.data_ptr(), gd.data_ptr(), M, C_out, N, h, w, 0, bw.data_ptr() if want_w else None,
                                     bb.data_ptr() if want_b else None, ws.data_ptr(), nbytes) == 0
        torch.cuda.synchronize()
        if want_w:
            assert bool((bb == PATTERN).all())
            assert_same(bw.view(torch.float32).reshape(C_out, M, 5, 5).cpu().numpy(), dW, "dW alone (ABI)")
        else:
            assert bool((bw == PATTERN).all())
            assert_same(bb.view(torch.float32).cpu().numpy(), db, "dbias alone (ABI)")
    # dbias alone does not read the anchors
    bb = torch.empty((C_out,), dtype=torch.float32, device=DEV)
    assert L.fgmm_ckbd_ctx_wgrad(ctx, None, None, gd.data_ptr(), M, C_out, N, h, w, 0, None, bb.data_ptr(), ws.data_ptr(), nbytes) == 0
    assert_same(bb.cpu().numpy(), db, "dbias without anchors")


def test_the_c_abi_refuses_and_writes_nothing():
    h, w, M, C_out, n = 3, 4, 2, 3, 2
    W, b, A, g = G.make_case(71, h, w, M, C_out, n)
    L, ctx = _lib.lib(), _lib.ctx(0)
    a, gd, wd = dv(A), dv(g), dv(W)
    guard = 64
    nw, nb, nbytes = C_out * M * 25, C_out, L.fgmm_ckbd_ctx_wgrad_workspace(M, C_out, n, h, w)
    nws = nbytes // 4
    nout, npk = n * C_out * h * (w // 2), L.fgmm_ckbd_ctx_packed_floats(M, C_out)
    sizes = [nws, nw, nb, nout, npk]  # (the workspace first: 16-byte aligned behind a guard of 64 words)
    buf = torch.full((guard + sum(s + guard for s in sizes),), PATTERN, dtype=torch.int32, device=DEV)
    starts = np.cumsum([guard] + [s + guard for s in sizes[:-1]])
    ws, dw, db, out, pk = (buf.data_ptr() + 4 * int(s) for s in starts)
    assert ws % 16 == 0
    torch.cuda.synchronize()

    def wgrad(anchors=a.data_ptr(), g_=gd.data_ptr(), M_=M, C_=C_out, n_=n, h_=h, w_=w, odd=0, dw_=dw, db_=db, ws_=ws, nbytes_=nbytes, ctx_=ctx):
        return L.fgmm_ckbd_ctx_wgrad(ctx_, None, anchors, g_, M_, C_, n_, h_, w_, odd, dw_, db_, ws_, nbytes_)

    refused = [dict(w_=5), dict(w_=0), dict(w_=-2), dict(h_=0), dict(n_=-1), dict(anchors=None), dict(g_=None), dict(odd=2), dict(ctx_=None),
               dict(M_=0), dict(C_=0), dict(h_=1 << 31, w_=4), dict(h_=1 << 24, w_=1 << 9), dict(h_=1 << 20, w_=1 << 9, n_=1 << 10),
               dict(dw_=None, db_=None), dict(ws_=None), dict(nbytes_=nbytes - 1), dict(nbytes_=0), dict(ws_=ws + 4), dict(dw_=dw + 2),
               dict(M_=1 << 20, C_=1 << 20, nbytes_=1 << 62)]  # (a grid of 98305 column groups x 32768 row tiles)
    for kw in refused:
        assert wgrad(**kw) == 1, kw  # FGMM_ERR_INVALID
        assert b"context convolution" in L.fgmm_last_error()

    def pack(weight=wd.data_ptr(), bias=None, M_=M, C_=C_out, tr=0, packed=pk, ctx_=ctx):
        return L.fgmm_ckbd_ctx_pack(ctx_, None, weight, bias, M_, C_, tr, packed)

    for kw in [dict(weight=None), dict(packed=None), dict(M_=0), dict(C_=-1), dict(tr=2), dict(tr=1, bias=dv(b).data_ptr()), dict(ctx_=None)]:
        assert pack(**kw) == 1, kw
        assert b"context convolution" in L.fgmm_last_error()

    def apply(packed=pk, M_=M, C_=C_out, anchors=a.data_ptr(), out_=out, n_=n, h_=h, w_=w, odd=0, ctx_=ctx):
        return L.fgmm_ckbd_ctx_apply_packed(ctx_, None, packed, M_, C_, anchors, out_, n_, h_, w_, odd)

    for kw in [dict(w_=5), dict(w_=0), dict(h_=0), dict(n_=-1), dict(anchors=None), dict(out_=None), dict(odd=2), dict(packed=None), dict(M_=0),
               dict(ctx_=None), dict(h_=1 << 31, w_=4), dict(h_=1 << 22, w_=1 << 9, n_=1 << 20)]:
        assert apply(**kw) == 1, kw
        assert b"context convolution" in L.fgmm_last_error()
    torch.cuda.synchronize()
    assert bool((buf == PATTERN).all())
    # n == 0 succeeds, with or without tensors, and launches nothing
    assert wgrad(n_=0) == 0 and wgrad(n_=0, anchors=None, g_=None, dw_=None, db_=None, ws_=None, nbytes_=0) == 0
    assert apply(n_=0) == 0 and apply(n_=0, anchors=None, out_=None, packed=None) == 0
    torch.cuda.synchronize()
    assert bool((buf == PATTERN).all())
    # ... and the accepted calls write their outputs between the guards, nothing else
    assert pack(bias=dv(b).data_ptr()) == 0 and apply() == 0 and wgrad() == 0
    torch.cuda.synchronize()
    inside = torch.zeros_like(buf, dtype=torch.bool)
    for s, size in zip(starts, sizes):
        inside[int(s):int(s) + size] = True
    assert bool((buf[~inside] == PATTERN).all())
    view = lambda s, size: buf[int(s):int(s) + size].view(torch.float32).cpu().numpy()  # noqa: E731
    kw_, kb_ = G.weight_grad(A, g, "even")
    assert_same(view(starts[1], nw).reshape(C_out, M, 5, 5), kw_, "dW")
    assert_same(view(starts[2], nb), kb_, "dbias")
    got = view(starts[3], nout).reshape(n, C_out, h, w // 2)
    for k in range(n):
        assert_same(got[k], R.chain(W, b, A[k], "even"), "apply_packed")


def test_the_calls_are_ordered_on_the_callers_stream(streams, delay):  # noqa: F811
    """the producers of the anchors and of g are still pending on the caller's stream when the calls are made; the results are consumed
    by work enqueued on that stream afterwards, and by another stream behind an event"""
    s1, s2, _ = streams
    case, parity = (5, 6, 32, 33, 1), "odd"
    W, b, A, g, dA, dW, db = reference(case, parity)
    _, _, A_d, g_d = G.make_case(82, *case)
    Wd = dv(W)
    want = [dv(dW), dv(db), dv(dA)]
    assert not np.array_equal(G.weight_grad(A_d, g_d, parity)[0], dW)
    with pending(s1, delay, [dv(A), dv(g)], [dv(A_d), dv(g_d)]) as (ab, gb):
        gw, gbias = wgrad_abi(ab, gb, parity)
        ga = dgrad_abi(Wd, gb, parity)
        twice = gw + gw  # enqueued after the call, on the same stream
        done = torch.cuda.Event()
        done.record()
        assert torch.equal(gw, want[0]) and torch.equal(gbias, want[1]) and torch.equal(ga, want[2]) and torch.equal(twice, want[0] + want[0])
        with torch.cuda.stream(s2):
            s2.wait_event(done)
            c2 = [gw.clone(), gbias.clone(), ga.clone()]
        s2.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(c2, want))


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_unembed_and_embed_are_differentiable(parity, dtype):
    """permutations: the gradients are the slicing form's autograd's, bit for bit; without a gradient asked for nothing changes"""
    torch.manual_seed(3)
    y = torch.randn((2, 3, 5, 6), device=DEV).to(dtype)
    gy_ = torch.randn((2, 2, 3, 5, 3), device=DEV).to(dtype)
    a, b = y.clone().requires_grad_(True), y.clone().requires_grad_(True)
    out = ckbd_unembed(a, parity)
    assert out.requires_grad and torch.equal(out, unembed_slices(b, parity))
    out.backward(gy_)
    unembed_slices(b, parity).backward(gy_)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.grad, ckbd_embed(gy_, parity))
    y_, gy = gy_, y
    a, b = y_.clone().requires_grad_(True), y_.clone().requires_grad_(True)
    out = ckbd_embed(a, parity)
    assert out.requires_grad and torch.equal(out, embed_slices(b, parity))
    out.backward(gy)
    embed_slices(b, parity).backward(gy)
    assert torch.equal(a.grad, b.grad) and torch.equal(a.grad, ckbd_unembed(gy, parity))
    assert not ckbd_unembed(y, parity).requires_grad and not ckbd_embed(y_, parity).requires_grad
    with torch.no_grad():
        assert not ckbd_unembed(y.clone().requires_grad_(True), parity).requires_grad


# ---- the codecs ------------------------------------------------------------------------------------------------------------------------
class MaskedConv(torch.nn.Conv2d):
    """the stand-in for the reference's CheckerboardMaskedConv2d, as tests/test_gpu_ckbd_context.py builds it"""

    def __init__(self, c_in, c_out, bias=True):
        super().__init__(c_in, c_out, 5, padding=2, bias=bias)
        self.register_buffer("mask", torch.from_numpy(R.masked(np.ones((c_out, c_in, 5, 5), np.float32))))

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.weight * self.mask, self.bias, padding=2)


class NeverRun(MaskedConv):
    def forward(self, x):
        raise AssertionError("the context convolution ran as a torch module")


def _ckbd_codec(M, seed, ctx_cls=MaskedConv, side=None, **kw):
    """a small checkerboard codec: context model a masked 5x5 convolution M -> 2 M, a pointwise parameter network, a K = 4 mixture"""
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    torch.manual_seed(seed)
    side = 2 * M if side is None else side
    ctx_net = ctx_cls(M, 2 * M)
    last = torch.nn.Conv2d(24, 12 * M, 1)
    with torch.no_grad():
        last.bias[: 4 * M] += 1.0  # sigma mostly positive
    ep = torch.nn.Sequential(torch.nn.Conv2d(2 * M + side, 24, 1), torch.nn.LeakyReLU(), last)
    return CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, mode="polya")}, entropy_parameters=ep,
                                   context_prediction=ctx_net, forward_method="onepass", **kw).to(DEV)


def _anchor_mask(h, w, parity):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[torch.arange(h)[:, None].expand(h, w // 2), torch.from_numpy(R.anchor_cols(h, w, parity))] = True
    return m.to(DEV)


def _grads(module):
    return {n: None if p.grad is None else p.grad.clone() for n, p in module.named_parameters()}


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("parity", R.PARITIES)
def test_checkerboard_forward_is_the_composition_of_its_parts(parity, training, capsys):
    M, C_out, h, w, B = 4, 8, 5, 6, 2
    rng = np.random.default_rng(11)
    y = dv((rng.standard_normal((B, M, h, w)) * 4).astype(np.float32))
    side = dv(rng.standard_normal((B, 2 * M, h, w)).astype(np.float32))
    anchors = _anchor_mask(h, w, parity)
    results = {}
    for fused in (False, True):
        codec = _ckbd_codec(M, 5, NeverRun if fused else MaskedConv, anchor_parity=parity, fuse_context=fused).train(training)
        seen = {}
        codec.context_prediction.register_forward_hook(lambda m, i, o: seen.__setitem__("ctx_in", i[0]))
        codec.entropy_parameters.register_forward_hook(lambda m, i, o: seen.__setitem__("ep", (i[0], o)))
        codec.latent_codec["y"].register_forward_hook(lambda m, i, o: seen.__setitem__("leaf", i))
        torch.manual_seed(99)
        out = codec(y, side)
        assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y"}
        y_hat, like = out["y_hat"], out["likelihoods"]["y"]
        assert like.shape == y.shape and y_hat.shape == y.shape
        if training:
            assert float((y_hat - y).abs().max()) <= 0.5 and not torch.equal(y_hat, torch.round(y))
        else:
            assert torch.equal(y_hat, torch.round(y))  # the checkerboard's own y_hat
        if not fused:
            assert seen["ctx_in"] is y_hat  # the context module is given y_hat
        ep_in, params = seen["ep"]
        y_ctx = ep_in[:, :C_out]
        assert ep_in.shape[1] == C_out + 2 * M and torch.equal(ep_in[:, C_out:], side)  # cat(y_ctx, side_params)
        assert not bool(y_ctx[:, :, anchors].any()) and bool(y_ctx[:, :, ~anchors].any())
        assert seen["leaf"][0] is y and seen["leaf"][1] is params  # latent_codec["y"](y, params)
        (-torch.log2(like)).sum().backward()
        results[fused] = (like.detach(), y_ctx.detach(), _grads(codec), y_hat.detach())
        if fused:
            # the same composition written out from the operator and the parts: the same bits, forward and backward
            twin = _ckbd_codec(M, 5, NeverRun, anchor_parity=parity, fuse_context=True).train(training)
            cp = twin.context_prediction
            torch.manual_seed(99)
            yh = y + torch.empty_like(y).uniform_(-0.5, 0.5) if training else torch.round(y)
            c1 = checkerboard_context(ckbd_unembed(yh, parity)[0], cp.weight * cp.mask, cp.bias, parity)
            yc = ckbd_embed(torch.stack([torch.zeros_like(c1), c1]), parity)
            o2 = twin.latent_codec["y"](y, twin.entropy_parameters(torch.cat([yc, side], 1)))
            (-torch.log2(o2["likelihoods"]["y"])).sum().backward()
            assert torch.equal(yh, y_hat) and torch.equal(yc.view(torch.int32), y_ctx.view(torch.int32))
            assert torch.equal(o2["likelihoods"]["y"].view(torch.int32), like.view(torch.int32))
            g1, g2 = results[True][2], _grads(twin)
            assert set(g1) == set(g2) and all(g1[n] is not None for n in g1 if n.startswith(("context_prediction.", "entropy_parameters.")))
            for name in g1:
                assert (g1[name] is None) == (g2[name] is None), name
                if g1[name] is not None:
                    assert torch.equal(g1[name].view(torch.int32), g2[name].view(torch.int32)), name
            gw = g1["context_prediction.weight"].reshape(C_out, M, 25)
            assert bool((gw[:, :, 0::2].view(torch.int32) == 0).all()) and bool((gw[:, :, 1::2] != 0).any())  # +0 at the dropped taps
    # fused against un-fused: the same y_hat; y_ctx within the chain's bound of each other; the likelihoods' difference printed only
    assert torch.equal(results[False][3], results[True][3])
    plain = _ckbd_codec(M, 5, MaskedConv, anchor_parity=parity)
    Wn = (plain.context_prediction.weight * plain.context_prediction.mask).detach().cpu().numpy()
    bn = plain.context_prediction.bias.detach().cpu().numpy()
    A_ = ckbd_unembed(results[True][3], parity)[0].cpu().numpy()
    c_f, c_u = (ckbd_unembed(results[f][1], parity)[1].cpu().numpy().astype(np.float64) for f in (True, False))
    for n in range(B):
        exact, bound = R.exact(Wn, bn, A_[n], parity), R.bound(Wn, bn, A_[n], parity)
        assert (np.abs(c_f[n] - exact) <= bound).all() and (np.abs(c_u[n] - exact) <= bound).all()
    with capsys.disabled():
        print(f"\n[ckbd forward {parity} {'train' if training else 'eval'}] |likelihood fused - un-fused| max "
              f"{float((results[True][0] - results[False][0]).abs().max()):.3e}")


def test_hyperprior_over_channel_groups_trains():
    """HyperpriorLatentCodec.forward over ChannelGroupsLatentCodec.forward over three fused checkerboard codecs, on a real
    EntropyBottleneck and real mixtures: keys, shapes, and which parameters the rate's gradient reaches"""
    from flashgmm_amd import EntropyBottleneck
    from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec, HyperLatentCodec, HyperpriorLatentCodec

    groups, h, w, B, Cz, side = [2, 2, 4], 6, 8, 2, 3, 6
    torch.manual_seed(21)
    hyper = HyperLatentCodec(entropy_bottleneck=EntropyBottleneck(Cz), h_a=torch.nn.Conv2d(8, Cz, 3, stride=2, padding=1),
                             h_s=torch.nn.ConvTranspose2d(Cz, side, 3, stride=2, padding=1, output_padding=1))
    cc = {"y1": torch.nn.Conv2d(2, 4, 1), "y2": torch.nn.Conv2d(4, 4, 1)}
    ys = {f"y{k}": _ckbd_codec(gk, 30 + k, NeverRun, side=side + (4 if k else 0), fuse_context=True) for k, gk in enumerate(groups)}
    codec = HyperpriorLatentCodec(latent_codec={"y": ChannelGroupsLatentCodec(latent_codec=ys, channel_context=cc, groups=groups), "hyper": hyper}).to(DEV)
    codec.train()
    y = (torch.randn((B, 8, h, w), device=DEV) * 3).requires_grad_(True)
    out = codec(y)
    assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y", "z"}
    assert out["likelihoods"]["y"].shape == y.shape and out["y_hat"].shape == y.shape
    assert out["likelihoods"]["z"].shape == (B, Cz, h // 2, w // 2)
    assert float((out["y_hat"] - y).detach().abs().max()) <= 0.5
    rate = sum((-torch.log2(v)).sum() for v in out["likelihoods"].values())
    rate.backward()
    eb = codec.latent_codec["hyper"].entropy_bottleneck
    assert y.grad is not None and bool((y.grad != 0).any())
    assert bool((codec.latent_codec["hyper"].h_a.weight.grad != 0).any()) and bool((codec.latent_codec["hyper"].h_s.weight.grad != 0).any())
    for k in range(3):
        gw = codec.latent_codec["y"].latent_codec[f"y{k}"].context_prediction.weight.grad
        flat = gw.reshape(gw.shape[0], gw.shape[1], 25)
        assert bool((flat[:, :, 1::2] != 0).any()) and bool((flat[:, :, 0::2].view(torch.int32) == 0).all())
    for k in (1, 2):
        assert bool((codec.latent_codec["y"].channel_context[f"y{k}"].weight.grad != 0).any())
    assert bool((eb._matrix0.grad != 0).any())
    assert eb.quantiles.grad is None or not bool(eb.quantiles.grad.any())  # the rate does not reach the quantiles ...
    eb.loss().backward()
    assert eb.quantiles.grad is not None and bool(eb.quantiles.grad.any())  # ... EntropyBottleneck.loss() does
