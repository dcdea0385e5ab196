"""CPU: the surface of the dense convolution's bf16x6 form (header section 5d, FGMM_CONV_BF16X6), and the classes refusing an unknown switch."""
import ctypes as C
import os
import re

import pytest
from torch import nn

from flashgmm_amd import ConvStack, _lib
from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec, HyperLatentCodec
from tests.test_conv_stack_cpu import channel_context, h_s


def test_the_surface_exists():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_CONV_BF16X6 1$", header, re.M) and _lib.FGMM_CONV_BF16X6 == 1 and re.search(r"^#define FGMM_HAS_CONV_BF16X6 1\b", header, re.M)
    p, i, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    for name, sig in {"fgmm_conv_create_ex": (i, [p, p, p, p, i, i, i, i, C.c_float, i, i, C.POINTER(p)]), "fgmm_conv_workspace_bytes": (sz, [p, i, i64]),
                      "fgmm_conv_apply_ws": (i, [p, p, p, p, i64, p, i, i, i, p, sz])}.items():
        assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == sig and name + "(" in header, name
    assert _lib.lib().fgmm_conv_workspace_bytes(None, 1, 16) == 0


def test_unknown_switches_are_refused():
    pytest.raises(ValueError, ConvStack, h_s(), arithmetic="fp8").match("arithmetic")
    elic_h_s = nn.Sequential(nn.ConvTranspose2d(8, 8, 5, stride=2, padding=2, output_padding=1), nn.ReLU(), nn.Conv2d(8, 8, 3, padding=1))
    pytest.raises(ValueError, ConvStack, elic_h_s, transposed=True, arithmetic="bf16x6").match("ConvTranspose2d")
    with pytest.raises(ValueError, match="ConvTranspose2d"):
        HyperLatentCodec(entropy_bottleneck=object(), h_s=elic_h_s, fuse_h_s="bf16x6")
    with pytest.raises(ValueError, match="fuse_h_s"):
        HyperLatentCodec(entropy_bottleneck=object(), h_s=h_s(), fuse_h_s="yes")
    with pytest.raises(ValueError, match="fuse_channel_context"):
        ChannelGroupsLatentCodec(latent_codec={}, channel_context={"y1": channel_context()}, groups=[12, 8], fuse_channel_context="yes")
    assert HyperLatentCodec(entropy_bottleneck=object(), h_s=h_s(), fuse_h_s="bf16x6")._h_s_arith == "bf16x6"
    assert ChannelGroupsLatentCodec(latent_codec={}, channel_context={"y1": channel_context()}, groups=[12, 8], fuse_channel_context="bf16x6")._cc_arith == "bf16x6"
