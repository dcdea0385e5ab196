"""CPU: the surface of the transposed convolution layers (header section 5e), the numpy definition against torch in float64, and what
ConvStack.check(transposed=True) takes and refuses before it touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from flashgmm_amd import ConvStack, _lib
from tests import conv_ref as R
from tests import deconv_ref as D

T = nn.ConvTranspose2d


def test_header_section_export_and_binding():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flashgmm_amd.h")).read()
    assert " 5e. " in header and re.search(r"^#define FGMM_HAS_CONV_TRANSPOSED 1\b", header, re.M)
    i, p = C.c_int, C.c_void_p
    name = "fgmm_conv_create_transposed"
    assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == (i, [p, p, p, p, i, i, i, i, i, C.c_float, C.POINTER(p)]) and name + "(" in header


@pytest.mark.parametrize("case", [D.CASES[3], D.CASES[4], D.CASES[7]], ids=str)
def test_the_definition_is_torch_s_transposed_convolution_within_the_bound(oracle, case):
    k, s, h, w, c_in, c_out, n, act = case
    W, b, x = D.make(sum(case), k, h, w, c_in, c_out, n)
    got = D.chain(oracle, W, b, x, s, act, 0.01)
    y = nn.functional.conv_transpose2d(torch.from_numpy(x).double(), torch.from_numpy(W).double(), torch.from_numpy(b).double(), stride=s, padding=k // 2,
                                       output_padding=s - 1)
    want = {R.NONE: lambda v: v, R.LEAKY: lambda v: nn.functional.leaky_relu(v, float(np.float32(0.01))), R.RELU: torch.relu}[act](y).numpy()
    bound = np.stack([D.bound(W, b, xi, s) for xi in x]) + 2.0**-24 * np.abs(want) + 2.0**-150
    assert got.shape == want.shape == (n, c_out, s * h, s * w) and (np.abs(got.astype(np.float64) - want) <= bound).all()


def elic_h_s(N=192):  # models/elic_gmm.py:142-148, deconv in models/utils.py:160-168
    deconv = lambda i, o, k, s: T(i, o, k, stride=s, padding=k // 2, output_padding=s - 1)
    return nn.Sequential(deconv(N, N, 5, 2), nn.ReLU(inplace=True), deconv(N, N * 3 // 2, 5, 2), nn.ReLU(inplace=True), deconv(N * 3 // 2, N * 2, 3, 1))


def test_check_takes_elic_s_h_s_and_mixed_stacks():
    layers = ConvStack.check(elic_h_s(), transposed=True)
    assert [(l[0].kernel_size[0], l[0].stride[0], l[1]) for l in layers] == [(5, 2, _lib.FGMM_ACT_RELU), (5, 2, _lib.FGMM_ACT_RELU), (3, 1, _lib.FGMM_ACT_NONE)]
    assert len(ConvStack.check([nn.ConvTranspose2d(4, 6, 3, stride=2, padding=1, output_padding=1), nn.ReLU(), nn.Conv2d(6, 4, 3, padding=1)], transposed=True)) == 2


@pytest.mark.parametrize("mods,reason", [
    ([T(4, 4, 5, stride=2, padding=2)], "output_padding"), ([T(4, 4, 3, stride=1, padding=0)], "padding == k // 2"),
    ([T(4, 4, 5, stride=3, padding=2, output_padding=2)], "stride"), ([T(4, 4, 4, stride=2, padding=2, output_padding=1)], "kernel of 3 or 5"),
    ([T(4, 4, 3, stride=2, padding=1, output_padding=1, groups=2)], "groups"), ([T(4, 4, 3, stride=1, padding=1, dilation=2)], "dilation"),
    ([T(4, 8, 5, stride=2, padding=2, output_padding=1), nn.ReLU(), T(4, 8, 3, padding=1)], "does not take the 8 channels")], ids=lambda v: v if isinstance(v, str) else "")
def test_check_refuses_a_transposed_layer_by_its_reason(mods, reason):
    with pytest.raises(ValueError, match="ConvStack.*" + re.escape(reason)):
        ConvStack.check(mods, transposed=True)


def test_the_hyper_codec_takes_elic_s_h_s_when_asked_to():
    from flashgmm_amd.latent_codecs import HyperLatentCodec

    codec = HyperLatentCodec(entropy_bottleneck=object(), h_s=elic_h_s(8), fuse_h_s="transposed")
    assert codec.fuse_h_s and codec._h_s_transposed
    with pytest.raises(ValueError, match="fuse_h_s"):
        HyperLatentCodec(entropy_bottleneck=object(), h_s=elic_h_s(8), fuse_h_s="yes")
