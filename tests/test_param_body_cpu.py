"""CPU: the surface of the parameter network's hidden layers (header section 2c) and what the two classes refuse before they touch a device."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch.nn as nn

from flashgmm_amd import ParameterBody, _lib
from flashgmm_amd.latent_codecs import CheckerboardLatentCodec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_surface_exists():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert " 2c. " in header and re.search(r"^#define FGMM_HAS_HIDDEN 1\b", header, re.M)
    assert [int(re.search(rf"^#define FGMM_ACT_{n} (\d)$", header, re.M).group(1)) for n in ("NONE", "LEAKY", "RELU")] == [
        _lib.FGMM_ACT_NONE, _lib.FGMM_ACT_LEAKY, _lib.FGMM_ACT_RELU] == [0, 1, 2]
    p, i = C.c_void_p, C.c_int
    for name, sig in {"fgmm_hidden_create": (i, [p, p, p, p, i, i, i, i, C.c_float, C.POINTER(p)]), "fgmm_hidden_destroy": (None, [p]),
                      "fgmm_hidden_apply": (i, [p, p, p, p, p, p, i, C.c_int64])}.items():
        assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == sig and name + "(" in header, name
    assert inspect.signature(CheckerboardLatentCodec.__init__).parameters["fuse_body"].default is False
    assert list(inspect.signature(ParameterBody.features).parameters)[1:] == ["ctx", "side"]


BAD = {"3x3": [nn.Conv2d(8, 8, 3, padding=1), nn.ReLU()], "grouped": [nn.Conv2d(8, 8, 1, groups=2)], "gelu": [nn.Conv2d(8, 8, 1), nn.GELU()],
       "two_activations": [nn.Conv2d(8, 8, 1), nn.ReLU(), nn.LeakyReLU()], "mismatch": [nn.Conv2d(8, 8, 1), nn.Conv2d(9, 8, 1)],
       "infinite_slope": [nn.Conv2d(8, 8, 1), nn.LeakyReLU(float("inf"))], "empty": []}


@pytest.mark.parametrize("mods", BAD.values(), ids=BAD.keys())
def test_what_does_not_fit_the_pattern_is_refused(mods):
    with pytest.raises(ValueError):
        ParameterBody(mods, 2)
    with pytest.raises(ValueError):
        CheckerboardLatentCodec(entropy_parameters=nn.Sequential(*mods, nn.Conv2d(8, 24, 1)), fuse_body=True)


def test_the_other_refusals():
    good = [nn.Conv2d(8, 8, 1), nn.LeakyReLU(0.2), nn.Conv2d(8, 8, 1)]
    for c_ctx in (8, 9, -1):  # a first layer no wider than the context
        with pytest.raises(ValueError, match="c_ctx"):
            ParameterBody(good, c_ctx)
    with pytest.raises(RuntimeError):  # CPU modules: no CPU implementation
        ParameterBody(good, 2)
    with pytest.raises(ValueError):  # not a Sequential of hidden layers and a last layer
        CheckerboardLatentCodec(entropy_parameters=nn.Conv2d(8, 24, 1), fuse_body=True)
    assert CheckerboardLatentCodec(entropy_parameters=nn.Sequential(*good, nn.ReLU(), nn.Conv2d(8, 24, 1)), fuse_body=True, fuse_head=True).fuse_body
