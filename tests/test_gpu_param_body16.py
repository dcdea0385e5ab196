"""GPU: the hidden layers' bf16x6 form (header section 2c, FGMM_HIDDEN_BF16X6; fgmm_hidden16.hip).  Bars: tests/hidden16_ref.py's bound of float64 at the kernel's edges; the same bits from every
launch, block height and place in a batch; an item outside the domain bit for bit the fmaf chain; the codec's strings those of a codec calling ParameterBody(arithmetic="bf16x6") itself."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import ParameterBody, _lib
from tests import hidden16_ref as R16
from tests import test_gpu_param_body as B
from tests.test_gpu_param_body import LEAKY, NONE, RELU, F32, chain, dv, height, make, same_bits

pytestmark = pytest.mark.gpu
L, bits = _lib.lib, lambda a: a.view(np.uint32)


def create16(W, b, c_a, act=NONE, slope=0.0, flags=_lib.FGMM_HIDDEN_BF16X6):
    h, Wd, bd = C.c_void_p(), dv(W), None if b is None else dv(b)
    rc = L().fgmm_hidden_create_ex(_lib.ctx(0), None, Wd.data_ptr(), None if b is None else bd.data_ptr(), W.shape[0], c_a, W.shape[1] - c_a, act, slope, flags, C.byref(h))
    return rc, h


def run16(W, b, xa, xb, act=NONE, slope=0.0, c_a=None, off=0):
    """the raw ABI, twice: W [c_out, c_a + c_b], xa [n, c_a, hw] or None (absent when c_a > 0), xb [n, c_b, hw] -> out [n, c_out, hw] (numpy)"""
    (n, _, hw), c_a = xb.shape, (0 if xa is None else xa.shape[1]) if c_a is None else c_a
    rc, h = create16(W, b, c_a, act, slope)
    assert rc == 0, L().fgmm_last_error()
    a_d, b_d = None if xa is None else dv(xa, off), dv(xb, off)
    need = L().fgmm_hidden_workspace_bytes(h, int(xa is not None), n, hw)
    ws, out = torch.empty(need, dtype=torch.uint8, device="cuda"), torch.full((n, W.shape[0], hw), float("nan"), device="cuda")
    got = []  # (twice: the same bits from every launch)
    for _ in range(2):
        rc = L().fgmm_hidden_apply_ws(_lib.ctx(0), None, h, None if xa is None else a_d.data_ptr(), b_d.data_ptr(), out.data_ptr(), n, hw, ws.data_ptr(), need)
        assert rc == 0, L().fgmm_last_error()
        got.append(out.cpu().numpy()), out.fill_(float("nan"))
    L().fgmm_hidden_destroy(h)
    assert np.array_equal(bits(got[0]), bits(got[1]))
    return got[0]


def assert_within(got, W, b, xa, xb, act, slope):
    refs = [R16.bound(W, b, None if xa is None else xa[i], xb[i], act, slope) for i in range(len(xb))]
    ratio = max(float((np.abs(g.astype(np.float64) - want) / bound).max()) for g, (want, bound) in zip(got, refs))
    print(f"largest err / bound {ratio:.3f}")
    assert ratio <= 1.0


# (c_a, c_b, c_out, hw, n, act, bias, absent, off): each source around the K tile of 16 (1, 15, 16, 17, 31, 33; a single source); c_out 1, 33
# and around the tallest block's 160 rows; positions 1, 3, 127 | 128 | 129 (the position tile's edge), 260; sources off the 16-byte grid
CASES = [(0, 1, 1, 1, 1, NONE, True, False, 0), (1, 31, 33, 3, 3, LEAKY, True, False, 0), (15, 17, 159, 127, 1, RELU, False, False, 0),
         (16, 16, 160, 128, 1, LEAKY, True, False, 0), (17, 15, 161, 129, 3, NONE, True, False, 0), (33, 31, 33, 260, 1, LEAKY, True, False, 0),
         (16, 17, 1, 260, 3, RELU, True, False, 1), (17, 16, 33, 128, 1, LEAKY, True, True, 0), (1, 31, 160, 3, 1, RELU, True, True, 0),
         (33, 15, 161, 260, 1, NONE, False, True, 1), (0, 1, 33, 127, 3, RELU, True, False, 0), (0, 17, 159, 129, 1, LEAKY, False, False, 0),
         (15, 16, 33, 1, 1, NONE, True, True, 0), (0, 31, 160, 260, 3, NONE, True, False, 0)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "a%d_b%d_o%d_hw%d_n%d_act%d_b%d_abs%d_off%d" % c)
def test_layer_is_within_the_derived_bound_of_float64(case):
    c_a, c_b, c_out, hw, n, act, bias, absent, off = case
    W, b, xa, xb = make(sum(case), c_a, c_b, c_out, hw, n, bias)
    got = run16(W, b, None if absent else xa, xb, act, 0.01, c_a, off)
    assert_within(got, W, b, None if absent else xa, xb, act, 0.01)
    if absent:  # finite weights, random biases: absent equals explicit zeros (a wrong tile offset into the packed weights would not)
        assert np.array_equal(bits(got), bits(run16(W, b, np.zeros_like(xa), xb, act, 0.01, c_a, off)))


@pytest.mark.parametrize("T,c_a,c_b,c_out,hw", [(5, 8, 8, 33, 32768), (5, 4, 4, 161, 16384), (2, 4, 4, 96, 16384), (1, 20, 20, 161, 260)], ids=lambda v: str(v))
def test_every_block_height_and_place_in_a_batch_gives_the_same_bits(T, c_a, c_b, c_out, hw):
    assert height(1, hw, c_out) == T and height(1, 260, c_out) == 1
    W, b, xa, xb = make(T + c_out, c_a, c_b, c_out, hw, 3)
    got = run16(W, b, xa, xb, LEAKY, 0.01)
    for i in range(3):  # every item of the batch has the bits it has alone
        assert np.array_equal(bits(run16(W, b, xa[i:i + 1], xb[i:i + 1], LEAKY, 0.01)[0]), bits(got[i]))
    low = run16(W, b, xa[:1, :, :260], xb[:1, :, :260], LEAKY, 0.01)  # the same elements from the shortest block
    assert np.array_equal(bits(low[0]), bits(got[0, :, :260]))
    assert_within(low, W, b, xa[:1, :, :260], xb[:1, :, :260], LEAKY, 0.01)


@pytest.mark.parametrize("src", ["a", "b"])
@pytest.mark.parametrize("v", [np.inf, np.nan, float.fromhex("0x1.FFp127")], ids=["inf", "nan", "edge"])
def test_an_item_outside_the_domain_is_the_fmaf_chain_and_a_weight_outside_is_refused(oracle, v, src):
    c_a, c_b, (W, b, xa, xb) = 17, 15, make(91, 17, 15, 33, 129, 3)
    (xa if src == "a" else xb)[1, 3, 128] = v
    got = run16(W, b, xa, xb, LEAKY, 0.01)
    assert same_bits(got[1], chain(oracle, W, b, xa[1:2], xb[1:2], LEAKY, 0.01, c_a)[0])
    for i in (0, 2):
        assert np.array_equal(bits(got[i]), bits(run16(W, b, xa[i:i + 1], xb[i:i + 1], LEAKY, 0.01)[0]))
        assert not np.array_equal(bits(got[i]), bits(chain(oracle, W, b, xa[i:i + 1], xb[i:i + 1], LEAKY, 0.01, c_a)[0]))  # (not the chain: the bf16x6 kernel's)
    W[32, 0 if src == "a" else c_a + c_b - 1] = v
    rc, h = create16(W, b, c_a)
    assert rc == 1 and not h.value and "domain" in str(L().fgmm_last_error())


def test_the_abi_refuses_what_the_header_says_and_writes_nothing():
    W, b, xa, xb = make(5, 4, 4, 8, 16, 1)
    assert all(create16(W, b, 4, flags=f)[0] == 1 and not create16(W, b, 4, flags=f)[1].value for f in (2, 3, -1))
    (_, h16), (_, exact) = create16(W, b, 4), create16(W, b, 4, flags=0)
    guarded, xa_d, xb_d = torch.full((3, 8, 16), float("nan"), device="cuda"), dv(xa), dv(xb)
    need = L().fgmm_hidden_workspace_bytes(h16, 1, 1, 16)
    assert need == (2 * 3 * 16 * 16 + 2 * 8) * 2 and [L().fgmm_hidden_workspace_bytes(*a) for a in [(h16, 0, 1, 16), (exact, 1, 1, 16), (h16, 1, 0, 16)]] == [need // 2, 0, 0]
    ws = torch.empty(need + 16, dtype=torch.uint8, device="cuda")
    apply_ws = lambda h, n, hw, *w: L().fgmm_hidden_apply_ws(_lib.ctx(0), None, h, xa_d.data_ptr(), xb_d.data_ptr(), guarded[1].data_ptr(), n, hw, *w)
    err = lambda: str(L().fgmm_last_error())
    assert L().fgmm_hidden_apply(_lib.ctx(0), None, h16, xa_d.data_ptr(), xb_d.data_ptr(), guarded[1].data_ptr(), 1, 16) == 1 and "fgmm_hidden_apply_ws" in err()
    assert apply_ws(h16, 1, 16, ws.data_ptr(), need - 1) == 1 and str(need) in err()  # one byte short
    assert apply_ws(h16, 1, 16, ws.data_ptr() + 4, need) == 1 and "aligned" in err()
    assert apply_ws(h16, 1, 16, None, need) == 1 and str(need) in err()
    assert apply_ws(h16, 0, 16, None, 0) == 0 and apply_ws(h16, 1, 0, None, 0) == 0  # nothing to do: no launch
    torch.cuda.synchronize()
    assert torch.isnan(guarded).all()
    assert apply_ws(exact, 1, 16, None, 0) == 0  # an exact handle ignores the workspace
    torch.cuda.synchronize()
    assert torch.isnan(guarded[0]).all() and torch.isnan(guarded[2]).all() and torch.isfinite(guarded[1]).all()
    L().fgmm_hidden_destroy(h16), L().fgmm_hidden_destroy(exact)


def test_apply_is_ordered_on_the_caller_s_stream(monkeypatch):
    # the delayed-producer case of the f32 test, its ParameterBody the bf16x6 one: the splits, both kernels and the workspace follow the stream
    monkeypatch.setattr(B, "ParameterBody", lambda mods, c_ctx: ParameterBody(mods, c_ctx, arithmetic="bf16x6"))
    B.test_apply_is_ordered_on_the_caller_s_stream()


def test_parameter_body_composes_the_layers_within_the_composed_bound():
    """|got - want| <= |W2| bound1 + bound2 at the first layer's own output; the f32 body 1e-5 of the largest output away at the most"""
    body = torch.manual_seed(4) and torch.nn.Sequential(torch.nn.Conv2d(40, 33, 1), torch.nn.LeakyReLU(0.2), torch.nn.Conv2d(33, 9, 1)).cuda()
    xa, xb = np.split(np.random.default_rng(6).standard_normal((2, 40, 35)).astype(F32), [8], 1)
    run = lambda mods, **kw: ParameterBody(mods, 8, **kw).features(*(torch.from_numpy(np.ascontiguousarray(a)).cuda().view(2, -1, 5, 7) for a in (xa, xb))).cpu().numpy().reshape(2, -1, 35)
    got, mid, f32 = run(body, arithmetic="bf16x6"), run(body[:2], arithmetic="bf16x6"), run(body)
    (W1, b1), (W2, b2) = [(m.weight.detach().cpu().numpy().reshape(m.out_channels, -1), m.bias.detach().cpu().numpy()) for m in (body[0], body[2])]
    for i in range(2):
        want1, bound1 = R16.bound(W1, b1, xa[i], xb[i], LEAKY, 0.2)
        want = R16.bound(W2, b2, None, want1, NONE, 0.0)[0]  # float64 all the way
        bound = np.abs(W2.astype(np.float64)) @ bound1 + R16.bound(W2, b2, None, mid[i], NONE, 0.0)[1]
        assert (np.abs(mid[i] - want1) <= bound1).all() and (np.abs(got[i] - want) <= bound).all()
    assert np.abs(got - f32).max() <= 1e-5 * np.abs(f32).max()


class Body16(B.BodyModule):  # entropy_parameters[:-1] calling ParameterBody(arithmetic="bf16x6") itself (the anchors' context: explicit zeros)
    def forward(self, x):
        return ParameterBody(self.mods, self.c_ctx, arithmetic="bf16x6").features(x[:, :self.c_ctx], x[:, self.c_ctx:])


@pytest.mark.parametrize("others", [False, "bf16x6"], ids=["alone", "with_head_and_context"])
def test_checkerboard_codec_with_the_bf16x6_body(monkeypatch, others):
    """the f32 test's checks (strings, decompress, decompress_many, silent hooks, repacking) with fuse_body="bf16x6" and Body16 in its place"""
    import flashgmm_amd.latent_codecs as LC

    real = LC.CheckerboardLatentCodec
    monkeypatch.setattr(LC, "CheckerboardLatentCodec", lambda **kw: real(**{**kw, "fuse_body": "bf16x6" if kw.get("fuse_body") else False}))
    monkeypatch.setattr(B, "BodyModule", Body16)
    B.test_checkerboard_codec_with_the_fused_body(others, others, "leaky")
