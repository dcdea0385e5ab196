"""The one item of tests/test_gpu_dec_frame.py, in numpy, so that tests/test_dec_frame_cpu.py can check without a GPU what that item
must be for the GPU test to mean anything: a decode-side kernel launched on a NEIGHBOURING rung of the ladder (another mode, the
other clamp flag) must decode other symbols than the coded ones.

(M, h, w) = (6, 8, 13): hw = 104 is a partial wave and a partial block.  The odd channels are all zero after rounding, so the compact
channel list and the dead channels matter; the even channels are coded: 3 * 104 = 312 symbols, one note at the smallest
checkpoint stride the library takes (256), two segments.  Sigma is left un-clamped by the generator and lies on both sides of the
clamp's lower bound 0.11 in the coded channels; abs_max is a few tens."""
from __future__ import annotations

import numpy as np

from tests import bf16_planes as B
from tests import synth as T

SHAPE = (6, 8, 13)  # the smallest M at which test_dec_frame_cpu.py passes (the issue's starting point: nothing had to be raised)
SEED = 18          # all three even channels coded, a tenth of their sigmas below 0.11, abs_max 44 (asserted by the CPU test)
STRIDE = 256        # the smallest checkpoint_stride GaussianMixtureConditional accepts and segdec_kernel is given
MODES = ("polya", "as", "logistic")
PLANES = ("float32", "float16", "bfloat16")


def make_item():
    """-> y, sigma, mu, pi as tests/synth.make_latent lays them out (sigma before the clamp), odd channels dead"""
    M, h, w = SHAPE
    y, sg, mu, pi = T.make_latent(SEED, M=M, h=h, w=w, clamp=False)
    y[0, 1::2] = np.float32(0.25)
    return y, sg, mu, pi


def planes(kind):
    """-> (what goes to the device: float32 / float16 arrays or bfloat16 bit patterns, the float32 values they widen to); the
    weights of the two-byte types are rounded toward zero (the sum of the widened weights must not exceed 1)"""
    _, sg, mu, pi = make_item()
    if kind == "float32":
        return (sg, mu, pi), (sg, mu, pi)
    if kind == "float16":
        p = T.to_float16_planes(sg, mu, pi)
        return p, tuple(a.astype(np.float32) for a in p)
    bits = B.planes_bits(sg, mu, pi, False)
    return bits, tuple(B.widen(b) for b in bits)


def coded(kind, clamp):
    """-> symbols, (sigma, mu, pi) rows as the coder gets them, abs_max, zero_bitmap, y_q"""
    y = make_item()[0]
    sym, s, m, w, am, zb, yq = T.to_coder_inputs(y, *planes(kind)[1], clamp=clamp)
    return sym, (s, m, w), am, zb, yq
