"""CPU: the bf16x6 context convolution's surface (header section 5b), and its bound (tests/ckbd_ctx16_ref.py) against an emulation."""
import os

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from tests import ckbd_ctx16_ref as R16
from tests import ckbd_ctx_ref as R
from tests import head_ref as H


def test_the_surface_exists_the_abi_version_stays_and_a_bad_arithmetic_is_refused():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flashgmm_amd.h")).read()
    assert "#define FGMM_CKBD_CTX_BF16X6 1" in header and "#define FGMM_ABI_VERSION 6 " in header
    for name in ("fgmm_ckbd_ctx_create_ex", "fgmm_ckbd_ctx_workspace_bytes", "fgmm_ckbd_ctx_apply_ws"):
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
    assert _lib.lib().fgmm_abi_version() == 6 and _lib.lib().fgmm_ckbd_ctx_workspace_bytes(None, 1, 4, 4) == 0
    # ... and a bad arithmetic is refused by the operator and by the codec
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec
    from flashgmm_amd.ops import CheckerboardContext

    conv = torch.nn.Conv2d(4, 8, 5, padding=2)
    with pytest.raises(ValueError, match="arithmetic"):
        CheckerboardContext(conv, "even", arithmetic="bf16")
    with pytest.raises(ValueError, match="fuse_context"):
        CheckerboardLatentCodec(fuse_context="bf16")
    got = [CheckerboardLatentCodec(fuse_context=v) for v in (False, True, "f32", "bf16x6")]
    assert [(c.fuse_context, c._context_arith) for c in got] == [(False, "f32"), (True, "f32"), (True, "f32"), (True, "bf16x6")]


@pytest.mark.parametrize("M", [c[2] for c in R16.CORPUS[-3:]])  # 15, 16, 17 at (5, 6), C_out = 33
def test_the_bound_covers_the_emulated_arithmetic_at_the_k_tile_s_edges(M):
    """from the bias, taps then 16-channel tiles of ONE tap ascending, six steps per tile, each one rounding of the accumulator"""
    W, b, A = R.make_case(400 + M, 5, 6, M, 33, 1)
    Ws, Xs = H.split3(R.pack(W)), H.split3(R.gather(A[0], "odd"))
    acc = np.zeros((33, 15), np.float32) + b[:, None]
    for k0 in (t * M + c0 for t in range(12) for c0 in range(0, M, 16)):
        k = slice(k0, min(k0 + 16, (k0 // M + 1) * M))
        for qa, qb in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)):
            acc = (acc.astype(np.float64) + Ws[qa][:, k].astype(np.float64) @ Xs[qb][k].astype(np.float64)).astype(np.float32)
    err, bound = np.abs(acc.reshape(33, 5, 3) - R.exact(W, b, A[0], "odd")), R16.bound(W, b, A[0], "odd")
    assert (err <= bound).all(), float((err / bound).max())
