"""CPU: the dense layers' gradients (header section 5f): the exports, the slice rule, the numpy definitions against float64 autograd, conv_layer's refusals."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import flashgmm_amd
from flashgmm_amd import _lib, ops
from tests import conv_grad_ref as G
from tests import conv_ref as R


def test_the_six_exports_are_bound():
    for name in ["fgmm_conv_packed_floats", "fgmm_conv_pack", "fgmm_conv_apply_packed", "fgmm_conv_dgrad", "fgmm_conv_wgrad_workspace", "fgmm_conv_wgrad"]:
        assert hasattr(_lib.lib(), name) and name in _lib.SIGNATURES, name
    assert flashgmm_amd.conv_layer is ops.conv_layer and "conv_layer" in ops.__all__ and _lib.lib().fgmm_conv_packed_floats(33, 9, 3) == 4 * 2 * 32 * 72 + 128
    assert (_lib.lib().fgmm_conv_wgrad_workspace(3, 2, 3, 1, 9, 29), _lib.lib().fgmm_conv_wgrad_workspace(3, 2, 4, 1, 9, 29)) == (2 * 3 * 19 * 4, 0)


def test_the_slice_rule_on_its_worked_values_and_a_sweep():
    worked = {(1, 1, 1): (1, 1), (1, 16, 16): (1, 2), (1, 9, 29): (2, 1), (2, 17, 33): (3, 2), (17, 16, 32): (12, 3)}
    assert {k: G.slices(*k) for k in worked} == worked and [len(at) for at in G.positions(1, 9, 29)] == [232, 29] and [len(at) for at in G.positions(17, 16, 32)][-1] == 256
    for n, h, w in [(n, h, w) for n in (1, 2, 3, 5, 40) for h in (1, 7, 8, 9, 31) for w in (1, 15, 16, 17, 50)]:
        (S, B), at = G.slices(n, h, w), G.positions(n, h, w)
        assert len(at) == S <= 16 and B * (S - 1) < n * -(-h // 8) <= B * S and np.array_equal(at[0][:min(w, 16)], np.arange(min(w, 16)))
        assert np.array_equal(np.sort(np.concatenate(at)), np.arange(n * h * w))  # every position once


@pytest.mark.parametrize("act,shuffle,k", [(a, s, k) for a in (R.NONE, R.LEAKY, R.RELU) for s in (1, 2) for k in (3, 5)])
def test_the_definitions_are_float64_autograd_within_the_bound(oracle, act, shuffle, k):
    """gz from the float64 forward's own output (both sides take the same branch); gy * slope: one more rounding.  (9, 29): two slices; c_out = 8: two shuffled planes"""
    n, c_in, c_out, h, w = 2, 3, 8, 9, 29
    W, b, x = R.make(act + shuffle + k, k, h, w, c_in, c_out, n)
    gy = np.random.default_rng(k).standard_normal((n, c_out // shuffle**2, h * shuffle, w * shuffle)).astype(R.F32)
    t = [torch.from_numpy(v).double().requires_grad_(True) for v in (x, W, b)]
    z = F.conv2d(*t, padding=k // 2)
    out = F.pixel_shuffle({R.NONE: lambda v: v, R.LEAKY: lambda v: F.leaky_relu(v, float(np.float32(0.01))), R.RELU: torch.relu}[act](z), shuffle)
    want = [v.numpy() for v in torch.autograd.grad(out, t, torch.from_numpy(gy).double())]
    g = G.gz(gy, out.detach().numpy().astype(R.F32), act, 0.01, shuffle)
    got = (G.data_grad(oracle, W, g),) + G.weight_grad(oracle, x, g, k)
    for v, ref, bound in zip(got, want, G.exact(x, W, g, extra=1)[1]):
        assert v.shape == ref.shape and (np.abs(v.astype(np.float64) - ref) <= bound + 2.0**-149).all()


def test_conv_layer_refuses_before_it_touches_a_device():
    x, w, b = torch.zeros(1, 4, 5, 5), torch.zeros(8, 4, 3, 3), torch.zeros(8)
    for kw, err in [(dict(activation="gelu"), ValueError), (dict(negative_slope=float("nan")), ValueError), (dict(activation="leaky_relu", negative_slope=-0.1), ValueError),
                    (dict(shuffle=3), ValueError), (dict(weight=torch.zeros(8, 4, 3, 5)), RuntimeError), (dict(weight=torch.zeros(6, 4, 3, 3), bias=None, shuffle=2), RuntimeError),
                    (dict(weight=w.double()), RuntimeError), (dict(bias=[0.0] * 8), TypeError), (dict(), RuntimeError)]:  # (the last: the weights are on the CPU)
        with pytest.raises(err):
            ops.conv_layer(**{**dict(x=x, weight=w, bias=b), **kw})
