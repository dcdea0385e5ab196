"""GPU: the dense convolution's bf16x6 form (header section 5d, FGMM_CONV_BF16X6; fgmm_conv16.hip).  Bars: small integers bit for bit
tests/conv_ref.py's chain (every product and partial sum is exact); tests/conv16_ref.py's bound of float64; the same bits from every block
height, place in a batch and launch; an item outside the domain bit for bit the exact handle's; the ABI's refusals; the codecs'
parameters those of ConvStack(arithmetic="bf16x6")."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import ConvStack, _lib
from tests import conv16_ref as R16
from tests import conv_ref as R
from tests import test_gpu_conv_stack as S
from tests.test_gpu_conv_stack import LEAKY, NONE, RELU, bits, dv, same_bits

pytestmark = pytest.mark.gpu
L = _lib.lib


def create16(W, b, act=NONE, slope=0.0, shuffle=1, flags=_lib.FGMM_CONV_BF16X6):
    hd, Wd, bd = C.c_void_p(), dv(W), None if b is None else dv(b)
    rc = L().fgmm_conv_create_ex(_lib.ctx(0), None, Wd.data_ptr(), None if b is None else bd.data_ptr(), W.shape[0], W.shape[1], W.shape[-1], act, slope, shuffle, flags,
                                 C.byref(hd))
    return rc, hd


def run16(W, b, x, act=NONE, slope=0.0, shuffle=1, wider=0):
    """the raw ABI, twice -> numpy; wider: x is the leading channels of a tensor with that many more, all NaN"""
    rc, hd = create16(W, b, act, slope, shuffle)
    assert rc == 0, L().fgmm_last_error()
    n, c_in, h, w = x.shape
    xd = dv(np.concatenate([x, np.full((n, wider, h, w), np.nan, R.F32)], 1))
    need = L().fgmm_conv_workspace_bytes(hd, n, h * w)
    ws, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.full((n, W.shape[0] // shuffle**2, h * shuffle, w * shuffle), float("nan"), device="cuda")
    got = []  # (twice: the same bits from every launch)
    for _ in range(2):
        rc = L().fgmm_conv_apply_ws(_lib.ctx(0), None, hd, xd.data_ptr(), (c_in + wider) * h * w, out.data_ptr(), n, h, w, ws.data_ptr(), need)
        assert rc == 0, L().fgmm_last_error()
        got.append(out.cpu().numpy()), out.fill_(float("nan"))
    L().fgmm_conv_destroy(hd)
    assert np.array_equal(bits(got[0]), bits(got[1]))
    return got[0]


# conv_ref's cases - the edges of the patch, the row tile and T - and the edges of the K tile of 16 channels with a padded last tile
@pytest.mark.parametrize("act", [NONE, RELU])
@pytest.mark.parametrize("case", R.CASES + [(5, 5, 6, c, 33, 1, 1, NONE) for c in (15, 16, 17, 33)], ids=str)
def test_small_integers_equal_the_chain_bit_for_bit(oracle, case, act):
    """weights, bias and inputs in [-8, 8]: every part product is exact and every partial sum below 2^24 (33 * 25 * 64 < 2^24)"""
    k, h, w, c_in, c_out, n, shuffle, _ = case
    r = np.random.default_rng(sum(case) + act)
    W, b, x = (r.integers(-8, 9, s).astype(R.F32) for s in ((c_out, c_in, k, k), (c_out,), (n, c_in, h, w)))
    b = None if c_out == 31 else b
    got = run16(W, b, x, act, 0.0, shuffle, wider=3 if c_in == 17 else 0)  # (the NaN channels beyond c_in are never read)
    want = R.chain(oracle, W, b, x, act, 0.0, shuffle)
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), np.abs(got - want).max()


@pytest.mark.parametrize("k,c_in", [(3, 400), (5, 130)])
def test_layer_is_within_the_derived_bound_of_float64(k, c_in):
    W, b, x = R.make(k + c_in, k, 9, 10, c_in, 16, 1)
    got = run16(W, b, x, LEAKY, 0.01)[0].reshape(16, -1).astype(np.float64)
    want, bound = R16.bound(W, b, x[0], LEAKY, 0.01)
    err = np.abs(got - want)
    print(f"k {k} K {c_in * k * k}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert (err <= bound).all()


# every height of the ladder, by the header's rule: B(T) = n * patches * ceil(row tiles / T) >= 256
@pytest.mark.parametrize("T,k,h,w,c_in,c_out", [(4, 3, 128, 256, 2, 129), (2, 5, 64, 256, 3, 65), (1, 3, 32, 64, 9, 33)], ids=str)
def test_every_block_height_and_place_in_a_batch_gives_the_same_bits(T, k, h, w, c_in, c_out):
    height = lambda hh, ww: next((t for t in (4, 2) if -(-hh // 8) * -(-ww // 16) * -(-(-(-c_out // 32)) // t) >= 256), 1)
    assert height(h, w) == T and height(11, 19) == 1
    W, b, x = R.make(T + c_out, k, h, w, c_in, c_out, 3)
    got, alone = run16(W, b, x, LEAKY, 0.01), run16(W, b, x[1:2], LEAKY, 0.01)
    assert np.array_equal(bits(alone[0]), bits(got[1]))  # an item alone has the bits it has inside a batch of three
    low = run16(W, b, x[1:2, :, :11, :19], LEAKY, 0.01)  # the same elements from the shortest block, away from the cut's halo
    assert np.array_equal(bits(low[0, :, :11 - k // 2, :19 - k // 2]), bits(got[1, :, :11 - k // 2, :19 - k // 2]))
    want, bound = R16.bound(W, b, x[1, :, :11, :19], LEAKY, 0.01)
    assert (np.abs(low[0].reshape(c_out, -1) - want) <= bound).all()


@pytest.mark.parametrize("k", [3, 5])
def test_an_item_outside_the_domain_is_the_exact_handle_s_and_a_weight_outside_is_refused(k):
    W, b, x = R.make(90 + k, k, 9, 17, 17, 33, 3)
    x[1, 0, 0, 0], x[1, 16, 8, 16], x[1, 5, 4, 9] = np.inf, np.nan, float.fromhex("0x1.FFp127")
    got, exact = run16(W, b, x, LEAKY, 0.01), S.run(W, b, x, LEAKY, 0.01)
    assert same_bits(got[1], exact[1])
    rest = run16(W, b, x[[0, 2]], LEAKY, 0.01)  # the other items: their bits from a call without item 1 - the bf16x6 kernel's, not the chain's
    assert np.array_equal(bits(got[[0, 2]]), bits(rest)) and not np.array_equal(bits(rest), bits(exact[[0, 2]]))
    for v in (np.inf, float.fromhex("0x1.FFp127")):
        Wv = W.copy()
        Wv[32, 16, k - 1, k - 1] = v
        rc, hd = create16(Wv, b)
        assert rc == 1 and not hd.value and "domain" in str(L().fgmm_last_error())


def test_the_abi_refuses_what_the_header_says_and_writes_nothing():
    W, b, x = R.make(5, 3, 4, 4, 4, 6, 1)
    assert all(create16(W, b, flags=f)[0] == 1 and not create16(W, b, flags=f)[1].value for f in (2, 3, -1))
    (_, h16), (_, exact) = create16(W, b), create16(W, b, flags=0)
    guarded, xd = torch.full((3, 6, 4, 4), float("nan"), device="cuda"), dv(x)
    need = L().fgmm_conv_workspace_bytes(h16, 1, 16)
    assert need == 3 * 16 * 16 * 2 + 16 and [L().fgmm_conv_workspace_bytes(*a) for a in [(exact, 1, 16), (h16, 0, 16), (h16, 1, 0)]] == [0, 0, 0]
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    apply_ws = lambda hd, n, h, *w: L().fgmm_conv_apply_ws(_lib.ctx(0), None, hd, xd.data_ptr(), 64, guarded[1].data_ptr(), n, h, 4, *w)
    err = lambda: str(L().fgmm_last_error())
    assert L().fgmm_conv_apply(_lib.ctx(0), None, h16, xd.data_ptr(), 64, guarded[1].data_ptr(), 1, 4, 4) == 1 and "fgmm_conv_apply_ws" in err()
    assert apply_ws(h16, 1, 4, ws.data_ptr(), need - 1) == 1 and str(need) in err()  # one byte short
    assert apply_ws(h16, 1, 4, ws.data_ptr() + 4, need) == 1 and "aligned" in err()
    assert apply_ws(h16, 1, 4, None, need) == 1 and str(need) in err()
    assert apply_ws(h16, 0, 4, None, 0) == 0 and apply_ws(h16, 1, 0, None, 0) == 0  # nothing to do: no launch
    torch.cuda.synchronize()
    assert torch.isnan(guarded).all()
    assert apply_ws(exact, 1, 4, None, 0) == 0 and apply_ws(h16, 1, 4, ws.data_ptr(), need) == 0  # an exact handle ignores the workspace
    torch.cuda.synchronize()
    assert torch.isnan(guarded[0]).all() and torch.isnan(guarded[2]).all() and torch.isfinite(guarded[1]).all()
    L().fgmm_conv_destroy(h16), L().fgmm_conv_destroy(exact)


@pytest.mark.parametrize("test", [S.test_apply_is_ordered_on_the_caller_s_stream, S.test_hyper_codec_with_the_fused_h_s,
                                  S.test_channel_groups_codec_with_the_fused_channel_context], ids=lambda t: t.__name__)
def test_the_f32_test_holds_with_bf16x6_in_every_place(monkeypatch, test):
    """the delayed-producer case and the two codec cases of the f32 tests (the parameters bit for bit ConvStack's, the torch modules
    silent, compress -> decompress round trips, repacking), their ConvStack and their codecs' switches the bf16x6 ones"""
    import flashgmm_amd.latent_codecs as LC

    made, hyper, groups = [], LC.HyperLatentCodec, LC.ChannelGroupsLatentCodec
    keep = lambda o: made.append(o) or o
    monkeypatch.setattr(S, "ConvStack", lambda mods: keep(ConvStack(mods, arithmetic="bf16x6")))
    monkeypatch.setattr(LC, "HyperLatentCodec", lambda **kw: keep(hyper(**{**kw, "fuse_h_s": "bf16x6"})))
    monkeypatch.setattr(LC, "ChannelGroupsLatentCodec", lambda **kw: keep(groups(**{**kw, "fuse_channel_context": "bf16x6"})))
    test()
    assert made and all("bf16x6" in (getattr(o, "arithmetic", None), getattr(o, "_h_s_arith", None), getattr(o, "_cc_arith", None)) for o in made)
    stacks = [s for o in made for _, s in list(getattr(o, "_h_s_stack", {}).values()) + list(getattr(o, "_cc_stacks", {}).values())]
    assert all(s.arithmetic == "bf16x6" for s in stacks) and (stacks or test is S.test_apply_is_ordered_on_the_caller_s_stream)
