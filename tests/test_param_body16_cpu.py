"""CPU: the surface of the hidden layers' bf16x6 form (header section 2c, FGMM_HIDDEN_BF16X6), and the two classes refusing an unknown switch."""
import ctypes as C
import os
import re

import pytest
import torch.nn as nn

from flashgmm_amd import ParameterBody, _lib
from flashgmm_amd.latent_codecs import CheckerboardLatentCodec


def test_the_surface_exists():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_HIDDEN_BF16X6 1$", header, re.M) and _lib.FGMM_HIDDEN_BF16X6 == 1 and re.search(r"^#define FGMM_HAS_HIDDEN_BF16X6 1\b", header, re.M)
    p, i, i64, sz = C.c_void_p, C.c_int, C.c_int64, C.c_size_t
    for name, sig in {"fgmm_hidden_create_ex": (i, [p, p, p, p, i, i, i, i, C.c_float, i, C.POINTER(p)]), "fgmm_hidden_workspace_bytes": (sz, [p, i, i, i64]),
                      "fgmm_hidden_apply_ws": (i, [p, p, p, p, p, p, i, i64, p, sz])}.items():
        assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == sig and name + "(" in header, name
    assert _lib.lib().fgmm_abi_version() == 6 and _lib.lib().fgmm_hidden_workspace_bytes(None, 1, 1, 16) == 0


@pytest.mark.parametrize("bad", ["bf16", "BF16X6", None, 2])
def test_an_unknown_arithmetic_is_refused(bad):
    mods = [nn.Conv2d(8, 8, 1), nn.LeakyReLU(0.2), nn.Conv2d(8, 8, 1)]
    pytest.raises(ValueError, ParameterBody, mods, 2, arithmetic=bad).match("arithmetic")
    with pytest.raises(ValueError, match="fuse_body"):
        CheckerboardLatentCodec(entropy_parameters=nn.Sequential(*mods, nn.ReLU(), nn.Conv2d(8, 24, 1)), fuse_body=bad)
    assert CheckerboardLatentCodec(entropy_parameters=nn.Sequential(*mods, nn.ReLU(), nn.Conv2d(8, 24, 1)), fuse_body="bf16x6")._body_arith == "bf16x6"
