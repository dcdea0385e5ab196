"""bfloat16 parameter planes (include/flashgmm_amd.h section 2, FGMM_BF16), the part that needs no GPU: the constants of the contract,
the test-side conversions of tests/bf16_planes.py against torch's, the precondition of the GPU tests' inputs, and the codec's argument."""
import os
import re

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from tests import bf16_planes as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_name_the_type():
    text = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define\s+FGMM_HAS_BF16\s+1\b", text, re.M)
    enum = re.search(r"typedef enum \{([^}]*)\} fgmm_dtype;", text).group(1)
    assert [e.strip() for e in enum.split(",")] == ["FGMM_F32 = 0", "FGMM_F16 = 1", "FGMM_BF16 = 2"]
    assert (_lib.FGMM_F32, _lib.FGMM_F16, _lib.FGMM_BF16) == (0, 1, 2)


def sweep():
    """float32 values that meet every case of the conversion: ties to even in both directions, the carry into the exponent and into
    infinity, subnormals (of binary32 and of bfloat16), both zeros, infinities, NaN, and random bit patterns"""
    rng = np.random.default_rng(5)
    pats = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,  # zeros, infinities, NaNs
            0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F818001, 0xBF808000, 0xBF818000,  # ties (even / odd keep), just off them
            0x3FFF8000, 0x3FFFFFFF, 0x7F7F8000, 0x7F7FFFFF, 0x7F7F7FFF,                          # carries: next exponent, infinity, not quite
            0x00000001, 0x00007FFF, 0x00008000, 0x00008001, 0x00018000, 0x007FFFFF, 0x00800000, 0x80008000, 0x807F8000]  # subnormals
    a = np.concatenate([np.array(pats, np.uint32), rng.integers(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32)])
    return a.view(np.float32)


def torch_bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_conversions_agree_with_torch():
    a = sweep()
    t = torch.from_numpy(a.copy())
    nan = np.isnan(a)
    got, want = B.bf16_rne(a), torch_bits(t.to(torch.bfloat16))
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(B.widen(got[nan])).all() and np.isnan(B.widen(want[nan])).all()
    # widening is torch's .float() of the same bits, bit for bit - NaN payloads included
    w = torch.from_numpy(got.view(np.int16).copy()).view(torch.bfloat16).to(torch.float32).numpy()
    assert np.array_equal(B.widen(got).view(np.uint32), w.view(np.uint32))
    assert np.array_equal(B.widen(got).view(np.uint32), got.astype(np.uint32) << 16)
    # toward zero: what is left after the low half is dropped converts exactly, and never grows in magnitude
    tr = B.bf16_trunc(a)
    masked = (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    assert np.array_equal(B.widen(tr).view(np.uint32), masked.view(np.uint32))
    fin = np.isfinite(a)
    assert np.array_equal(torch_bits(torch.from_numpy(masked[fin].copy()).to(torch.bfloat16)), tr[fin])
    assert (np.abs(B.widen(tr)[fin]) <= np.abs(a[fin])).all()


def test_truncated_weights_of_every_gpu_input_sum_to_at_most_one():
    """the precondition of the two-byte forms, checked in the kernels' own order of summation, (p0 + p1) + (p2 + p3) in binary32"""
    for name, (y, sg, mu, pi) in B.items().items():
        _, _, wb = B.planes_bits(sg, mu, pi, logits=False)
        p = B.widen(wb).reshape(4, -1)
        s = (p[0] + p[1]) + (p[2] + p[3])
        assert s.dtype == np.float32 and (s <= np.float32(1.0)).all(), name
        assert (p >= 0).all() and (p <= pi.reshape(4, -1)).all(), name
    # ... which round-to-nearest weights do not meet: the reason the helper truncates
    y, sg, mu, pi = B.items()["v8_linear"]
    p = B.widen(B.bf16_rne(pi)).reshape(4, -1)
    assert ((p[0] + p[1]) + (p[2] + p[3]) > np.float32(1.0)).any()


def test_codec_accepts_bfloat16_planes():
    from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec

    codec = GaussianMixtureConditionalLatentCodec(K=4, param_dtype=torch.bfloat16)
    assert codec.param_dtype == torch.bfloat16
    for bad in (torch.float64, torch.int16):
        with pytest.raises(ValueError, match="bfloat16"):
            GaussianMixtureConditionalLatentCodec(K=4, param_dtype=bad)
    with pytest.raises(ValueError):  # fuse_softmax keeps its float32-only rule at codec level
        GaussianMixtureConditionalLatentCodec(K=4, param_dtype=torch.bfloat16, fuse_softmax=True)
    # _planes: sigma and mu to nearest, the weights toward zero - the test-side helper's bits
    y, sg, mu, pi = B.items()["v8_tiled"]
    s, m, w = codec._planes(*(torch.from_numpy(a) for a in (sg, mu, pi)))
    assert s.dtype == m.dtype == w.dtype == torch.bfloat16
    for got, want in zip((s, m, w), B.planes_bits(sg, mu, pi, logits=False)):
        assert np.array_equal(torch_bits(got.contiguous()), want)
