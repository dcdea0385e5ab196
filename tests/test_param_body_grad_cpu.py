"""CPU: the surface of the hidden layers' gradients (header section 2d): the macro, the six exports and their bindings, and
flashgmm_amd.ops.pointwise_layer's refusals that need no GPU.  tests/test_gpu_param_body_grad.py holds the kernels to their definitions."""
import ctypes as C
import os
import re

import pytest
import torch

from flashgmm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_surface_exists():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert " 2d. " in header and re.search(r"^#define FGMM_HAS_HIDDEN_GRAD 1\b", header, re.M)
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M) and _lib.lib().fgmm_abi_version() == 6  # added without a bump
    p, i, i64, sz, f = C.c_void_p, C.c_int, C.c_int64, C.c_size_t, C.c_float
    want = {
        "fgmm_hidden_packed_floats": (sz, [i, i, i]),
        "fgmm_hidden_pack": (i, [p, p, p, p, i, i, i, i, p]),
        "fgmm_hidden_apply_packed": (i, [p, p, p, i, i, i, i, f, p, p, p, i, i64]),
        "fgmm_hidden_dgrad": (i, [p, p, p, i, i, i, i, f, p, p, p, p, i, i64]),
        "fgmm_hidden_wgrad_workspace": (sz, [i, i, i, i, i, i64]),
        "fgmm_hidden_wgrad": (i, [p, p, p, p, p, p, i, i, i, i, f, i, i64, p, p, p, sz]),
    }
    for name, sig in want.items():
        assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == sig and name + "(" in header, name


def test_the_operator_refuses_what_it_cannot_run():
    import flashgmm_amd
    from flashgmm_amd import ops

    assert flashgmm_amd.pointwise_layer is ops.pointwise_layer and "pointwise_layer" in ops.__all__
    ctx, side, W, b = torch.zeros(1, 2, 3, 4), torch.zeros(1, 3, 3, 4), torch.zeros(6, 5), torch.zeros(6)
    with pytest.raises(ValueError):
        ops.pointwise_layer(ctx, side, W, b, activation="gelu")
    with pytest.raises(ValueError):  # the saved output's sign would not be the pre-activation's
        ops.pointwise_layer(ctx, side, W, b, activation="leaky_relu", negative_slope=-0.1)
    with pytest.raises(RuntimeError):  # CPU tensors: no CPU fallback
        ops.pointwise_layer(ctx, side, W, b)
