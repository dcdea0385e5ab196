"""bfloat16 parameter planes for the tests (include/flashgmm_amd.h section 2, FGMM_BF16), in numpy: the conversions, and the inputs that
tests/test_gpu_bf16_planes.py runs - kept here so that tests/test_bf16_planes_cpu.py can check, without a GPU, the precondition those
inputs must meet (after widening, sum_k pi_k <= 1).

A bfloat16 value is the upper half of a binary32 pattern.  sigma and mu are rounded to nearest even, pi is rounded TOWARD ZERO (the low
half dropped), and widening is `<< 16`: exact, NaN payloads, infinities, signed zeros and subnormals kept."""
from __future__ import annotations

import numpy as np

from tests import synth as T


def bf16_rne(a) -> np.ndarray:
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even; a NaN becomes the quiet NaN 0x7FC0, as torch's conversion makes it"""
    bits = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    out = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(np.asarray(a, np.float32))] = 0x7FC0
    return out


def bf16_trunc(a) -> np.ndarray:
    """float32 -> bfloat16 bit patterns, rounded toward zero: the low 16 bits dropped"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def widen(bits) -> np.ndarray:
    """bfloat16 bit patterns -> the float32 values they stand for"""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------------------------
# (M, h, w) -> the form of the encode-side kernels an item of that shape reaches when it is a call of its own (the ladders of
# fgmm_encode.cpp enqueue_kernels and fgmm_estimate.cpp LatentFrame::start)
SHAPES = {
    "v8_linear": (5, 16, 32),  # hw = 512: compress 8-wide on the linear grid; the frame calls 4-wide, linear
    "v8_tiled": (5, 8, 12),    # hw = 96: 8-wide and 4-wide, tiled grid
    "v4_only": (5, 3, 4),      # hw = 12: no multiple of 8 - 4-wide, 8-byte loads
    "v1_tiled": (5, 15, 17),   # hw = 255: 1-wide, tiled
    "v1_linear": (5, 8, 8),    # hw = 64, given as views two bytes into their storage: 1-wide, linear
}
OFFSET_VIEW = ("v1_linear",)   # shapes whose planes the GPU tests hand over misaligned
SEGDEC_SHAPE = (40, 16, 12)
DEAD, OUTLIER = 1, 3           # channel without a coded symbol; channel with one latent the coder bypasses


def make_item(seed: int, M: int, h: int, w: int, outlier: float = 200.0):
    """-> y, sigma, mu, pi as tests/synth.make_latent lays them out (sigma before the clamp), with channel DEAD all zero after rounding and
    one latent of channel OUTLIER far outside a narrow mixture: its pmf quantises to 0 and the coder takes the bypass escape"""
    y, sg, mu, pi = T.make_latent(seed, M=M, h=h, w=w, clamp=False)
    y[0, DEAD] = np.float32(0.25)
    y[0, OUTLIER, 0, 1] = np.float32(outlier)
    for k in range(4):
        sg[0, k * M + OUTLIER, 0, 1] = np.float32(0.2)
        mu[0, k * M + OUTLIER, 0, 1] = np.float32(0.0)
    return y, sg, mu, pi


def make_special(seed: int = 77):
    """the item with special values, shape v8_tiled: sigma at 1e-5 and at 3e3 (both outside the clamp), a subnormal mean, -0.0, a NaN sigma"""
    M, h, w = SHAPES["v8_tiled"]
    y, sg, mu, pi = make_item(seed, M, h, w)
    sg[0, 0 * M + 0, 0, 0] = np.float32(1e-5)
    sg[0, 1 * M + 0, 0, 1] = np.float32(3e3)
    mu[0, 0 * M + 2, 1, 0] = np.float32(1e-40)
    mu[0, 1 * M + 2, 1, 1] = np.float32(-0.0)
    sg[0, 2 * M + 4, 2, 2] = np.float32(np.nan)
    return y, sg, mu, pi


def planes_bits(sg, mu, pi, logits: bool):
    """-> the three planes as bfloat16 bit patterns: sigma and mu to nearest; the weights toward zero, or - logits - log(pi) to nearest"""
    if logits:
        return bf16_rne(sg), bf16_rne(mu), bf16_rne(np.log(pi).astype(np.float32))
    return bf16_rne(sg), bf16_rne(mu), bf16_trunc(pi)


def items():
    """name -> (y, sigma, mu, pi): every input of tests/test_gpu_bf16_planes.py that is made here"""
    out = {name: make_item(100 + i, *shape) for i, (name, shape) in enumerate(SHAPES.items())}
    out["special"] = make_special()
    out["wide"] = make_item(120, 4, 8, 12, outlier=600.0)  # abs_max = 601: a half-width above 511, the generic cdftab form
    out["segdec"] = make_item(121, *SEGDEC_SHAPE)
    for i in range(3):
        out[f"stack{i}"] = make_item(130 + i, *SHAPES["v8_tiled"])
    return out
