"""CPU: the surface of the context convolution's gradients (header section 5c, the five exports, flashgmm_amd.ops.checkerboard_context,
the three codecs' forward()), the slice rule, and the restatement (tests/ckbd_ctx_grad_ref.py) - which the GPU tests hold the kernels to
bit for bit - against torch autograd in float64 of conv2d(embed([A, noise]), W * mask, b, padding=2) read at the non-anchors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from tests import ckbd_ctx_grad_ref as G
from tests import ckbd_ctx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = dict(ids=lambda c: "h%d_w%d_M%d_C%d_N%d" % c)


def test_the_surface_exists():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert " 5c. " in header and re.search(r"^#define FGMM_HAS_CKBD_CONTEXT_GRAD 1\b", header, re.M)
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M) and _lib.lib().fgmm_abi_version() == 6  # added without a bump
    L = _lib.lib()
    p, i, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    want = {
        "fgmm_ckbd_ctx_packed_floats": (sz, [i, i]),
        "fgmm_ckbd_ctx_pack": (i, [p, p, p, p, i, i, i, p]),
        "fgmm_ckbd_ctx_apply_packed": (i, [p, p, p, i, i, p, p, i, i64, i64, i]),
        "fgmm_ckbd_ctx_wgrad_workspace": (sz, [i, i, i, i64, i64]),
        "fgmm_ckbd_ctx_wgrad": (i, [p, p, p, p, i, i, i, i64, i64, i, p, p, p, sz]),
    }
    for name, sig in want.items():
        assert hasattr(L, name) and _lib.SIGNATURES[name] == sig, name
    # the slice constants: the header states them, the binding and the restatement restate them
    lo = int(re.search(r"^#define FGMM_CKBD_WGRAD_SLICE_MIN (\d+)\b", header, re.M).group(1))
    hi = int(re.search(r"^#define FGMM_CKBD_WGRAD_SLICES_MAX (\d+)\b", header, re.M).group(1))
    assert (lo, hi) == (G.SLICE_MIN, G.SLICES_MAX) == (_lib.FGMM_CKBD_WGRAD_SLICE_MIN, _lib.FGMM_CKBD_WGRAD_SLICES_MAX)
    assert "layers.py:141-144" in header  # the difference from the reference is stated where the arithmetic is
    import flashgmm_amd
    from flashgmm_amd import ops

    assert flashgmm_amd.checkerboard_context is ops.checkerboard_context and "checkerboard_context" in ops.__all__
    assert "layers.py:141-144" in ops.CheckerboardContext.__doc__ and "layers.py:141-144" in ops.checkerboard_context.__doc__


def test_the_sizes_the_library_reports_need_no_gpu():
    """packed_floats and wgrad_workspace are host arithmetic: the forward's packing (row tiles padded to six, K tiles of 32), and S
    partial copies of [C_out, 12 M + 1] float32"""
    L = _lib.lib()
    for M, C_out in ((1, 1), (33, 193), (192, 384)):
        n_rt, mt = -(-(-(-C_out // 32)) // 6) * 6, -(-M // 32)
        assert L.fgmm_ckbd_ctx_packed_floats(M, C_out) == n_rt * 12 * mt * 1024 + n_rt * 32
        for n, h, w in ((1, 1, 2), (3, 9, 30), (17, 16, 32), (24, 32, 48)):
            S, _ = G.slices(n * h * (w // 2))
            assert L.fgmm_ckbd_ctx_wgrad_workspace(M, C_out, n, h, w) == S * C_out * (12 * M + 1) * 4
    assert L.fgmm_ckbd_ctx_wgrad_workspace(192, 384, 24, 32, 48) == 16 * 384 * 2305 * 4  # 57 MB: the bound the cap of 16 sets
    assert L.fgmm_ckbd_ctx_packed_floats(0, 4) == 0 and L.fgmm_ckbd_ctx_wgrad_workspace(2, 3, 1, 4, 5) == 0  # refused sizes
    assert L.fgmm_ckbd_ctx_wgrad_workspace(2, 3, 0, 4, 6) == 0


def test_the_slice_rule():
    assert G.slices(1) == (1, 32) and G.slices(405) == (2, 224)
    assert G.slices(4097) == (15, 288)  # the sixteenth slice would be empty
    assert G.slices(4352) == (16, 288) and G.slice_ranges(4352)[-1] == (4320, 4352)  # the last slice 32 long
    for P in range(1, 5001):
        S, L = G.slices(P)
        r = G.slice_ranges(P)
        assert 1 <= S <= 16 and L % 32 == 0 and len(r) == S
        assert r[0][0] == 0 and r[-1][1] == P and all(a < b for a, b in r)  # no empty slice
        assert all(r[k][1] == r[k + 1][0] for k in range(S - 1))  # a cover without overlap


def test_the_corpus_holds_what_it_claims():
    assert set(R.CORPUS) <= set(G.CORPUS) and len(set(G.CORPUS)) == len(G.CORPUS)
    P = {c: c[4] * c[0] * (c[1] // 2) for c in G.CORPUS}
    assert P[(9, 30, 2, 3, 3)] == 405 and G.slices(405)[0] == 2
    assert all(0 < b < 224 or 224 < b < 405 for b in (135, 270))  # both item boundaries inside a slice, none on a slice's edge
    assert P[(16, 32, 2, 3, 17)] == 4352 and G.slices(4352) == (16, 288) and 4352 - 15 * 288 == 32
    assert P[(1, 2, 1, 1, 1)] == 1
    assert {G.slices(p)[0] for p in P.values()} >= {1, 2, 16}
    assert any(p % 32 for p in P.values())  # a last chunk that is not full


def _autograd64(W, b, A, g, parity, noise, mask_in_graph=True):
    """float64 autograd of sum(g * conv2d(embed([A, noise]), W (* mask), b, padding=2) at the non-anchors) -> dA, dW, db (numpy)"""
    N, M, h, w2 = A.shape
    r = torch.arange(h)[:, None].expand(h, w2)
    a_cols, n_cols = torch.from_numpy(R.anchor_cols(h, 2 * w2, parity)), torch.from_numpy(R.non_anchor_cols(h, 2 * w2, parity))
    At = torch.from_numpy(A).double().requires_grad_(True)
    Wt = torch.from_numpy(W).double().requires_grad_(True)
    bt = torch.from_numpy(b).double().requires_grad_(True)
    full = torch.zeros((N, M, h, 2 * w2), dtype=torch.float64)
    full[:, :, r, n_cols] = torch.from_numpy(noise).double()
    full[:, :, r, a_cols] = At  # (autograd follows the assignment)
    mask = torch.from_numpy(R.masked(np.ones_like(W))).double()
    out = torch.nn.functional.conv2d(full, Wt * mask if mask_in_graph else Wt, bt, padding=2)
    (out[:, :, r, n_cols] * torch.from_numpy(g).double()).sum().backward()
    return At.grad.numpy(), Wt.grad.numpy(), bt.grad.numpy()


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("case", [(2, 2, 2, 31, 3), (3, 4, 31, 32, 1), (5, 6, 32, 33, 1), (9, 30, 2, 3, 3), (1, 2, 1, 1, 1)], **IDS)
def test_the_restated_gradients_are_autograd_s_in_float64(case, parity):
    """in float64 every binary32 product is exact: the restatement's sums and autograd's differ by their summation orders alone - two
    sums of n terms each within (n - 1) 2^-53 sum |terms| of the exact one - n = 12 C_out for dA, the P positions for dW and dbias"""
    h, w, M, C_out, N = case
    W, b, A, g = G.make_case(400 + h + M, h, w, M, C_out, N)
    noise = np.random.default_rng(3).standard_normal(A.shape).astype(np.float32) * 50  # the non-anchor half: read by nobody
    dA, dW, db = _autograd64(W, b, A, g, parity, noise)
    P = N * h * (w // 2)
    for n in range(N):
        gap = 12 * C_out * 2.0**-52 * G.data_grad_abs(W, g[n], parity)
        assert (np.abs(G.data_grad_exact(W, g[n], parity) - dA[n]) <= gap).all()
    (ew, eb), (aw, ab) = G.weight_grad_exact(A, g, parity), G.weight_grad_abs(A, g, parity)
    assert (np.abs(ew - dW) <= P * 2.0**-52 * aw).all() and (np.abs(eb - db) <= P * 2.0**-52 * ab).all()
    # ... and the definitions themselves (binary32 chains, binary32 adds of the slices) are within their bound of those sums
    S, L = G.slices(P)
    kw, kb = G.weight_grad(A, g, parity)
    assert kw.dtype == kb.dtype == np.float32
    assert (np.abs(kw - ew) <= R.H.gamma(L + S) * aw).all() and (np.abs(kb - eb) <= R.H.gamma(L + S) * ab).all()
    dropped = np.ones((5, 5), bool)
    for i, j in R.TAPS:
        dropped[i, j] = False
    assert (kw[:, :, dropped].view(np.uint32) == 0).all()  # +0 at the 13 dropped taps
    for n in range(N):
        k = G.data_grad(W, g[n], parity)
        assert (np.abs(k - G.data_grad_exact(W, g[n], parity)) <= R.bound(G.flip_transpose(W), None, g[n], G.other(parity))).all()


def test_the_documented_difference_from_the_reference():
    """the reference zeroes weight.data and differentiates a PLAIN convolution: its dropped taps get gradients; weight * mask's get 0"""
    h, w, M, C_out, N = 5, 6, 2, 3, 2
    W, b, A, g = G.make_case(77, h, w, M, C_out, N)
    noise = np.random.default_rng(5).standard_normal(A.shape).astype(np.float32)
    _, dW_masked, _ = _autograd64(W, b, A, g, "even", noise)
    _, dW_plain, _ = _autograd64(W, b, A, g, "even", noise, mask_in_graph=False)  # (W is masked already: the same forward values)
    dropped = np.ones((5, 5), bool)
    for i, j in R.TAPS:
        dropped[i, j] = False
    assert (dW_masked[:, :, dropped] == 0).all() and (dW_plain[:, :, dropped] != 0).any()
    assert np.array_equal(dW_masked[:, :, ~dropped], dW_plain[:, :, ~dropped])
    assert (G.weight_grad(A, g, "even")[0][:, :, dropped] == 0).all()


# ---- Python refusals that need no GPU ------------------------------------------------------------------------------------------------
def test_the_operator_refuses_what_it_cannot_run():
    from flashgmm_amd.ops import checkerboard_context, ckbd_embed, ckbd_unembed

    A, W, b = torch.zeros(1, 2, 3, 2), torch.zeros(3, 2, 5, 5), torch.zeros(3)
    with pytest.raises(RuntimeError):  # CPU tensors: no CPU fallback
        checkerboard_context(A, W, b)
    with pytest.raises(RuntimeError):
        checkerboard_context(A, W.double(), b)
    with pytest.raises(RuntimeError):
        checkerboard_context(A, torch.zeros(3, 2, 3, 3), b)
    with pytest.raises(RuntimeError):
        checkerboard_context(A, torch.zeros(3, 2, 25), b)
    with pytest.raises(ValueError):
        checkerboard_context(A, W, b, anchor_parity="both")
    with pytest.raises(TypeError):
        checkerboard_context(A.numpy(), W, b)
    # the permutations, with an input that asks for a gradient: refused like one that does not
    for fn, t in ((ckbd_unembed, torch.zeros(1, 2, 4, 4, requires_grad=True)), (ckbd_embed, torch.zeros(2, 1, 2, 4, 2, requires_grad=True))):
        with pytest.raises(RuntimeError):
            fn(t)
        with pytest.raises(ValueError):
            fn(t, "both")


# ---- the codecs' forward() over stand-in modules ------------------------------------------------------------------------------------
class MaskedConv(torch.nn.Conv2d):
    """the stand-in for the reference's CheckerboardMaskedConv2d, as tests/test_gpu_ckbd_context.py builds it"""

    def __init__(self, c_in, c_out):
        super().__init__(c_in, c_out, 5, padding=2)
        self.register_buffer("mask", torch.from_numpy(R.masked(np.ones((c_out, c_in, 5, 5), np.float32))))

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.weight * self.mask, self.bias, padding=2)


class Leaf(torch.nn.Module):
    """a stand-in for latent_codec["y"]: records what it is called with, returns a likelihood and a y_hat that name the call"""

    def __init__(self, tag=0.0):
        super().__init__()
        self.tag, self.calls = tag, []

    def forward(self, y, params):
        self.calls.append((y, params))
        return {"likelihoods": {"y": torch.sigmoid(y + params[:, : y.shape[1]])}, "y_hat": torch.round(y) + self.tag}


def _ckbd_codec(M=2, C_out=4, **kw):
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec

    torch.manual_seed(0)
    return CheckerboardLatentCodec(latent_codec={"y": Leaf()}, entropy_parameters=torch.nn.Conv2d(C_out + 3, M, 1),
                                   context_prediction=kw.pop("context", MaskedConv(M, C_out)), forward_method=kw.pop("forward_method", "onepass"), **kw)


@pytest.mark.parametrize("parity", R.PARITIES)
def test_checkerboard_forward_is_the_reference_s_one_pass(parity):
    M, C_out, h, w, B = 2, 4, 5, 6, 2
    codec = _ckbd_codec(M, C_out, anchor_parity=parity)
    y, side = torch.randn(B, M, h, w) * 3, torch.randn(B, 3, h, w)
    seen = {}
    codec.context_prediction.register_forward_hook(lambda m, i, o: seen.__setitem__("ctx_in", i[0]))
    codec.entropy_parameters.register_forward_hook(lambda m, i, o: seen.__setitem__("ep", (i[0], o)))
    anchors = torch.zeros(h, w, dtype=torch.bool)
    anchors[torch.arange(h)[:, None].expand(h, w // 2), torch.from_numpy(R.anchor_cols(h, w, parity))] = True
    for training in (False, True):
        codec.train(training)
        out = codec(y, side)
        assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y"}
        y_hat = out["y_hat"]
        if training:
            assert float((y_hat - y).abs().max()) <= 0.5 and not torch.equal(y_hat, torch.round(y))
        else:
            assert torch.equal(y_hat, torch.round(y))
        assert seen["ctx_in"] is y_hat  # the context model is given the checkerboard's own y_hat
        ep_in, params = seen["ep"]
        y_ctx = ep_in[:, :C_out]
        assert torch.equal(ep_in[:, C_out:], side) and ep_in.shape[1] == C_out + 3  # merge(y_ctx, side_params), in that order
        assert not bool(y_ctx[:, :, anchors].any())
        assert torch.equal(y_ctx[:, :, ~anchors], codec.context_prediction(y_hat)[:, :, ~anchors])
        got_y, got_params = codec.latent_codec["y"].calls[-1]
        assert got_y is y and got_params is params  # latent_codec["y"](y, params): y, not y_hat
        assert torch.equal(out["likelihoods"]["y"], torch.sigmoid(y + params[:, :M]))
    # the gradient reaches the context model's weight through weight * mask: zero at the dropped taps
    codec.eval()
    codec(y, side)["likelihoods"]["y"].sum().backward()
    gw = codec.context_prediction.weight.grad
    assert bool((gw.reshape(C_out, M, 25)[:, :, 0::2] == 0).all()) and bool((gw.reshape(C_out, M, 25)[:, :, 1::2] != 0).any())


def test_checkerboard_forward_refuses():
    y, side = torch.zeros(1, 2, 4, 4), torch.zeros(1, 3, 4, 4)
    for method in ("twopass", "twopass_faster"):
        with pytest.raises(NotImplementedError, match=r"ckbd_gmm\.py:125"):
            _ckbd_codec(forward_method=method)(y, side)
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec

    assert CheckerboardLatentCodec().forward_method == "twopass"  # the constructor's default stays the reference's
    for fuse in (False, True):
        with pytest.raises(ValueError):  # no mask buffer
            _ckbd_codec(context=torch.nn.Conv2d(2, 4, 5, padding=2), fuse_context=fuse)(y, side)
        bad = MaskedConv(2, 4)
        bad.mask[1, 1, 2, 2] = 1.0  # the centre tap: not the checkerboard pattern
        with pytest.raises(ValueError):
            _ckbd_codec(context=bad, fuse_context=fuse)(y, side)
        bad = MaskedConv(2, 4)
        bad.mask[0, 0, 0, 1] = 0.0  # a kept tap masked out
        with pytest.raises(ValueError):
            _ckbd_codec(context=bad, fuse_context=fuse)(y, side)
    with pytest.raises(RuntimeError):  # fuse_context on CPU tensors: the operator has no CPU fallback
        _ckbd_codec(fuse_context=True)(y, side)


def test_channel_groups_forward_is_the_reference_s():
    from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec

    groups, h, w, B = [2, 2, 4], 3, 4, 2
    torch.manual_seed(1)
    leaves = {f"y{k}": Leaf(tag=0.25 * (k + 1)) for k in range(3)}
    cc = {"y1": torch.nn.Conv2d(2, 5, 1), "y2": torch.nn.Conv2d(4, 5, 1)}
    codec = ChannelGroupsLatentCodec(latent_codec=leaves, channel_context=cc, groups=groups)
    y, side = torch.randn(B, 8, h, w) * 3, torch.randn(B, 6, h, w)
    seen = {}
    for k in (1, 2):
        cc[f"y{k}"].register_forward_hook(lambda m, i, o, k=k: seen.__setitem__(k, (i[0], o)))
    out = codec(y, side)
    assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y"}
    parts = torch.split(y, groups, dim=1)
    hats = [torch.round(parts[k]) + 0.25 * (k + 1) for k in range(3)]
    assert torch.equal(out["y_hat"], torch.cat(hats, 1))  # concatenated in group order
    for k in range(3):
        (gy, gp), = leaves[f"y{k}"].calls
        assert torch.equal(gy, parts[k])
        if k == 0:
            assert gp is side
        else:  # the channel context sees the y_hat of groups 0 .. k-1, and precedes the side parameters
            assert torch.equal(seen[k][0], torch.cat(hats[:k], 1))
            assert torch.equal(gp, torch.cat([seen[k][1], side], 1))
    like = torch.cat([torch.sigmoid(parts[k] + leaves[f"y{k}"].calls[0][1][:, : groups[k]]) for k in range(3)], 1)
    assert torch.equal(out["likelihoods"]["y"], like)


def test_hyperprior_forward_is_the_reference_s():
    from flashgmm_amd.latent_codecs import HyperpriorLatentCodec

    class Hyper(torch.nn.Module):
        def forward(self, y):
            return {"likelihoods": {"z": y[:, :1] * 0 + 0.5}, "params": y * 2}

    leaf = Leaf(tag=0.125)
    codec = HyperpriorLatentCodec(latent_codec={"y": leaf, "hyper": Hyper()})
    y = torch.randn(2, 3, 4, 4)
    out = codec(y)
    assert set(out) == {"likelihoods", "y_hat"} and set(out["likelihoods"]) == {"y", "z"}
    (gy, gp), = leaf.calls
    assert gy is y and torch.equal(gp, y * 2)
    assert torch.equal(out["y_hat"], torch.round(y) + 0.125) and torch.equal(out["likelihoods"]["z"], y[:, :1] * 0 + 0.5)
    assert torch.equal(out["likelihoods"]["y"], torch.sigmoid(y + 2 * y))
