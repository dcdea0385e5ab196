"""GPU (-m gpu): the checkerboard context convolution in bf16x6 (header section 5b, FGMM_CKBD_CTX_BF16X6; fgmm_ckbd_ctx16.hip)."""
import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from flashgmm_amd.ops import CheckerboardContext
from tests import ckbd_ctx16_ref as R16
from tests import ckbd_ctx_ref as R
from tests.test_gpu_ckbd_context import DEV, NeverRun, _codec, _latent, _row_tiles_per_block, assert_is_the_chain, dv, module_of
from tests.test_gpu_streams import delay, pending, streams  # noqa: F401  (the fixtures and THE helper of the stream tests)

pytestmark = pytest.mark.gpu
EDGE = float.fromhex("0x1.FFp127")


def op16(W, b, parity):
    return CheckerboardContext(module_of(W, b), parity, arithmetic="bf16x6")


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_within_the_bound(got, W, b, A, parity):
    err, bound = np.abs(got.cpu().numpy().astype(np.float64) - R.exact(W, b, A, parity)), R16.bound(W, b, A, parity)
    print(f"largest error {float((err / bound).max()):.4f} of the bound")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("case", R16.CORPUS, ids=lambda c: "h%d_w%d_M%d_C%d_N%d" % c)
def test_the_operator_is_within_the_bound_of_float64_and_repeats_its_bits(case, parity):
    h, w, M, C_out, N = case
    W, b, A = R.make_case(500 + h + M, h, w, M, C_out, N)
    op = op16(W, b, parity)
    got = op.non_anchor(dv(A))
    for n in range(N):
        assert_within_the_bound(got[n], W, b, A[n], parity)
    assert same_bits(op.non_anchor(dv(A)), got)


def test_every_launch_form_gives_an_item_the_bits_it_has_alone():
    """the launcher's rule is the f32 kernel's: at 135 positions (two tiles) and C_out = 193 (seven row tiles) the smallest N of each height"""
    W, b, A = R.make_case(600, 9, 30, 33, 193, 64)
    op, a = op16(W, b, "odd"), dv(A)
    alone = torch.cat([op.non_anchor(a[k:k + 1]) for k in range(64)])
    for N, T in ((1, 1), (32, 2), (64, 6)):
        assert _row_tiles_per_block(N, 9, 30, 193) == T and (N == 1 or _row_tiles_per_block(N - 1, 9, 30, 193) != T)
        assert same_bits(op.non_anchor(a[64 - N:]), alone[64 - N:]), N  # (an item's place in the batch changes with N too)


@pytest.mark.parametrize("planted", [np.inf, np.nan, EDGE], ids=["inf", "nan", "edge"])
def test_a_flagged_item_is_the_exact_chain_and_its_neighbours_are_untouched(planted):
    W, b, A = R.make_case(700, 5, 6, 33, 33, 3)
    A[1, 17, 2, 1] = planted
    op = op16(W, b, "even")
    got = op.non_anchor(dv(A))
    assert_is_the_chain(got[1:2].cpu().numpy(), W, b, A[1:2], "even")
    for k in (0, 2):
        assert same_bits(got[k], op.non_anchor(dv(A[k:k + 1]))[0])
        assert_within_the_bound(got[k], W, b, A[k], "even")
    W[3, 5, 0, 1] = EDGE  # a kept tap
    with pytest.raises(_lib.FgmmError, match="domain"):
        op16(W, b, "even")


def test_the_c_abi_refuses_and_writes_nothing():
    h, w, M, C_out, n = 3, 4, 17, 3, 2
    W, b, A = R.make_case(800, h, w, M, C_out, n)
    op, a, L, ctx = op16(W, b, "even"), dv(A), _lib.lib(), _lib.ctx(0)
    need = L.fgmm_ckbd_ctx_workspace_bytes(op._h, n, h, w)
    assert need == n * (2 * 3 * 2 * 16 * h * (w // 2) + 16) and L.fgmm_ckbd_ctx_workspace_bytes(CheckerboardContext(module_of(W, b))._h, n, h, w) == 0
    guard, body, pattern = 64, n * C_out * h * (w // 2), 0x7FC12345
    out, ws = (torch.full((guard + k + guard,), pattern, dtype=torch.int32, device=DEV) for k in (body, need // 4))
    o_ptr, w_ptr = out.data_ptr() + 4 * guard, ws.data_ptr() + 4 * guard
    for wsp, nbytes in ((None, need), (w_ptr, need - 1), (w_ptr + 4, need + 64)):  # null, short, misaligned
        assert L.fgmm_ckbd_ctx_apply_ws(ctx, None, op._h, a.data_ptr(), o_ptr, n, h, w, 0, wsp, nbytes) == 1 and str(need).encode() in L.fgmm_last_error()
    assert L.fgmm_ckbd_ctx_apply(ctx, None, op._h, a.data_ptr(), o_ptr, n, h, w, 0) == 1 and b"fgmm_ckbd_ctx_apply_ws" in L.fgmm_last_error()
    torch.cuda.synchronize()
    assert bool((out == pattern).all()) and bool((ws == pattern).all())
    assert L.fgmm_ckbd_ctx_apply_ws(ctx, None, op._h, a.data_ptr(), o_ptr, n, h, w, 0, w_ptr, need) == 0
    torch.cuda.synchronize()
    for buf, size in ((out, body), (ws, need // 4)):
        assert bool((buf[:guard] == pattern).all()) and bool((buf[guard + size:] == pattern).all())
    assert same_bits(out[guard:guard + body].view(torch.float32).reshape(n, C_out, h, w // 2), op.non_anchor(a))


def test_the_call_is_ordered_on_the_callers_stream(streams, delay):  # noqa: F811
    (W, b, A), A_d = R.make_case(900, 5, 6, 32, 33, 1), R.make_case(901, 5, 6, 32, 33, 1)[2]
    op = op16(W, b, "odd")
    want = op.non_anchor(dv(A))
    assert not same_bits(want, op.non_anchor(dv(A_d)))
    with pending(streams[0], delay, [dv(A)], [dv(A_d)]) as (ab,):  # the anchors' producer is still pending on the caller's stream
        got = op.non_anchor(ab)
        assert same_bits(got, want) and torch.equal(got + got, want + want)


def test_a_codec_codes_a_batch_and_decodes_its_items_one_by_one():  # (NeverRun: the context module's forward raises)
    codec = _codec(24, 5, NeverRun, fuse_context="bf16x6")
    assert codec._context_op().arithmetic == "bf16x6"
    items = [_latent(24, 10, 14, 10 + k) for k in range(3)]
    with torch.no_grad():
        alone = [codec.compress(y, side) for y, side in items]
        batched = codec._ctx(torch.cat([codec.unembed(a["y_hat"]) for a in alone], 1), 1)  # the three anchors halves as ONE batch
        for k, ((y, side), a) in enumerate(zip(items, alone)):
            assert same_bits(batched[k:k + 1], codec._ctx(codec.unembed(a["y_hat"]), 1))
            assert torch.equal(codec.decompress(a["strings"], a["shape"], side)["y_hat"], a["y_hat"]) and torch.equal(a["y_hat"], torch.round(y))
