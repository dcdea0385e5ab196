"""CPU: the surface of the dense convolution layers (header section 5d), the numpy definition against torch in float64, and what
ConvStack.check takes and refuses before it touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from flashgmm_amd import ConvStack, _lib
from tests import conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_section_exports_and_binding():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert " 5d. " in header and re.search(r"^#define FGMM_HAS_CONV 1\b", header, re.M)
    i, p, i64 = C.c_int, C.c_void_p, C.c_int64
    for name, sig in {"fgmm_conv_create": (i, [p, p, p, p, i, i, i, i, C.c_float, i, C.POINTER(p)]), "fgmm_conv_destroy": (None, [p]),
                      "fgmm_conv_apply": (i, [p, p, p, p, i64, p, i, i, i])}.items():
        assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == sig and name + "(" in header, name


@pytest.mark.parametrize("case", R.CASES[1:7], ids=str)
def test_the_definition_is_torch_s_convolution_within_the_bound(oracle, case):
    k, h, w, c_in, c_out, n, shuffle, act = case
    W, b, x = R.make(sum(case), k, h, w, c_in, c_out, n)
    got = R.chain(oracle, W, b, x, act, 0.01, shuffle)
    y = nn.functional.conv2d(torch.from_numpy(x).double(), torch.from_numpy(W).double(), torch.from_numpy(b).double(), padding=k // 2)
    y = {R.NONE: lambda v: v, R.LEAKY: lambda v: nn.functional.leaky_relu(v, float(np.float32(0.01))), R.RELU: torch.relu}[act](y)
    want = nn.functional.pixel_shuffle(y, shuffle).numpy()
    bound = np.stack([R.shuffled(R.bound(W, b, xi).reshape(-1, h, w), shuffle) for xi in x]) + 2.0**-24 * np.abs(want) + 2.0**-150
    assert got.shape == want.shape and (np.abs(got.astype(np.float64) - want) <= bound).all()


def h_s(N=8, M=16):  # models/ckbd_gmm.py:97-107
    conv3 = lambda i, o: nn.Conv2d(i, o, 3, padding=1)
    subpel = lambda i, o: nn.Sequential(nn.Conv2d(i, o * 4, 3, padding=1), nn.PixelShuffle(2))
    return nn.Sequential(conv3(N, M), nn.LeakyReLU(inplace=True), subpel(M, M), nn.LeakyReLU(inplace=True), conv3(M, M * 3 // 2), nn.LeakyReLU(inplace=True),
                         subpel(M * 3 // 2, M * 3 // 2), nn.LeakyReLU(inplace=True), conv3(M * 3 // 2, M * 2))


def channel_context(c_in=12, c_out=8):  # models/elic_gmm.py:151-164
    conv5 = lambda i, o: nn.Conv2d(i, o, 5, padding=2)
    return nn.Sequential(conv5(c_in, 224), nn.ReLU(inplace=True), conv5(224, 128), nn.ReLU(inplace=True), conv5(128, c_out * 2))


def test_check_takes_the_two_reference_modules():
    layers = ConvStack.check(h_s())
    assert [(l[0].kernel_size[0], l[1], l[3]) for l in layers] == [(3, 1, 1), (3, 1, 2), (3, 1, 1), (3, 1, 2), (3, 0, 1)]
    assert abs(layers[0][2] - 0.01) < 1e-9
    assert [(l[0].kernel_size[0], l[1], l[3]) for l in ConvStack.check(channel_context())] == [(5, 2, 1), (5, 2, 1), (5, 0, 1)]


@pytest.mark.parametrize("mods", [
    [nn.Conv2d(4, 4, 3, stride=2, padding=1)], [nn.ConvTranspose2d(4, 4, 5, stride=2, padding=2, output_padding=1)], [nn.Conv2d(4, 4, 1)],
    [nn.Conv2d(4, 4, 3, padding=0)], [nn.Conv2d(4, 4, 3, padding=1, groups=2)], [nn.Conv2d(4, 4, 3, padding=1, padding_mode="reflect")],
    [nn.Conv2d(4, 4, 3, padding=2, dilation=2)], [nn.Conv2d(4, 4, (3, 5), padding=(1, 2))], [nn.Sequential(nn.Conv2d(4, 9, 3, padding=1), nn.PixelShuffle(3))],
    [nn.Sequential(nn.Conv2d(4, 6, 3, padding=1), nn.PixelShuffle(2))], [nn.Conv2d(4, 8, 3, padding=1), nn.Conv2d(4, 8, 3, padding=1)],
    [nn.Sequential(nn.Conv2d(4, 8, 3, padding=1), nn.PixelShuffle(2)), nn.Conv2d(8, 4, 3, padding=1)], [nn.Conv2d(4, 4, 3, padding=1), nn.LeakyReLU(float("nan"))],
    [nn.Conv2d(4, 4, 3, padding=1), nn.ReLU(), nn.ReLU()], [nn.ReLU()], []], ids=lambda m: (type(m[0]).__name__ if m else "empty"))
def test_check_refuses_what_does_not_fit(mods):
    with pytest.raises(ValueError, match="ConvStack"):
        ConvStack.check(mods)


def test_the_codecs_refuse_a_module_the_stack_does_not_take():
    from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec, HyperLatentCodec

    elic_h_s = nn.Sequential(nn.ConvTranspose2d(8, 8, 5, stride=2, padding=2, output_padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1))
    with pytest.raises(ValueError, match="ConvTranspose2d"):
        HyperLatentCodec(entropy_bottleneck=object(), h_s=elic_h_s, fuse_h_s=True)
    with pytest.raises(ValueError, match="ConvStack"):
        ChannelGroupsLatentCodec(latent_codec={}, channel_context={"y1": nn.Sequential(nn.Conv2d(4, 4, 1))}, groups=[4, 4], fuse_channel_context=True)
    assert not HyperLatentCodec(entropy_bottleneck=object(), h_s=elic_h_s).fuse_h_s  # (off by default: any h_s)
