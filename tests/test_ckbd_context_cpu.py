"""CPU: the checkerboard context convolution's surface (header section 5b, the three exports, the Python classes) and its restatement
(tests/ckbd_ctx_ref.py) - which the GPU tests hold fgmm_ckbd_ctx.hip to bit for bit - against the thing it restates: the reference's
unembed(context_prediction(embed([anchors, 0])))[1] with a masked 5x5 convolution, in float64 where only the summation order differs."""
import inspect
import os

import numpy as np
import pytest
import torch

from flashgmm_amd import _lib
from tests import ckbd_ctx_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_surface_exists():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert " 5b. " in header and "#define FGMM_HAS_CKBD_CONTEXT 1" in header
    L = _lib.lib()
    for name in ("fgmm_ckbd_ctx_create", "fgmm_ckbd_ctx_destroy", "fgmm_ckbd_ctx_apply"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec
    from flashgmm_amd.ops import CheckerboardContext

    assert callable(CheckerboardContext.non_anchor)
    assert list(inspect.signature(CheckerboardContext.__init__).parameters)[1:] == ["conv", "anchor_parity"]
    assert inspect.signature(CheckerboardLatentCodec.__init__).parameters["fuse_context"].default is False


def test_the_tap_list_is_the_issue_s():
    assert R.TAPS == [(0, 1), (0, 3), (1, 0), (1, 2), (1, 4), (2, 1), (2, 3), (3, 0), (3, 2), (3, 4), (4, 1), (4, 3)]
    assert [5 * i + j for i, j in R.TAPS] == [2 * t + 1 for t in range(12)]  # what the kernels compute the tap from


def _torch_path(W, b, A, parity, fill=None):
    """unembed(conv2d(embed([A, fill or 0]), W, b, padding=2))[1] in float64, for one item A [M, h, w/2] -> [C_out, h, w/2]"""
    M, h, w2 = A.shape
    rows = torch.arange(h)[:, None].expand(h, w2)
    a_cols, n_cols = torch.from_numpy(R.anchor_cols(h, 2 * w2, parity)), torch.from_numpy(R.non_anchor_cols(h, 2 * w2, parity))
    full = torch.zeros((1, M, h, 2 * w2), dtype=torch.float64)
    full[0][:, rows, a_cols] = torch.from_numpy(A).double()
    if fill is not None:
        full[0][:, rows, n_cols] = torch.from_numpy(fill).double()
    out = torch.nn.functional.conv2d(full, torch.from_numpy(W).double(), None if b is None else torch.from_numpy(b).double(), padding=2)
    return out[0][:, rows, n_cols].numpy()


@pytest.mark.parametrize("parity", R.PARITIES)
@pytest.mark.parametrize("case", R.CORPUS, ids=lambda c: "h%d_w%d_M%d_C%d_N%d" % c)
def test_the_restatement_is_the_masked_convolution_between_embed_and_unembed(case, parity):
    """in float64 every binary32 product is exact, so the restatement and torch's convolution differ by their two summation orders and
    nothing else: at most 12 M 2^-52 sum |w x| without a bias (two recursive sums of 12 M non-zero terms, each within (12 M - 1) 2^-53
    sum |w x| of the exact sum); with a bias there is one more term in either sum: 12 M 2^-52 (sum |w x| + |b|)"""
    h, w, M, C_out, N = case
    W, b, A = R.make_case(100 + h + M, h, w, M, C_out, N)
    for n in range(N):
        for bias in (None, b):
            want = _torch_path(W, bias, A[n], parity)
            got = R.exact(W, bias, A[n], parity)
            gap = 12 * M * 2.0**-52 * R.H.abs_sum(R.pack(W), bias, R.gather(A[n], parity)).reshape(want.shape)
            assert got.shape == want.shape == (C_out, h, w // 2)
            assert (np.abs(got - want) <= gap).all(), np.abs(got - want).max()
        # ... and what the non-anchor half holds does not matter: to the convolution (the mask), nor to the restatement (it never sees it)
        fill = np.random.default_rng(7).standard_normal(A[n].shape).astype(np.float32) * 100
        assert (np.abs(_torch_path(W, b, A[n], parity, fill) - want) <= gap).all()


@pytest.mark.parametrize("parity", R.PARITIES)
def test_the_restatement_reads_the_anchors_half_only(parity):
    """its only inputs are the weights, the bias and the anchors half: gather() indexes A and nothing else, and every index it uses
    inside the image is an anchor's (asserted in neighbours())"""
    for h, w, *_ in R.CORPUS:
        nb = R.neighbours(h, w, parity)
        assert nb.shape == (12, h * (w // 2)) and nb.max() < h * (w // 2) and nb.min() >= -1
    A = np.arange(2 * 3 * 2, dtype=np.float32).reshape(2, 3, 2) + 1
    X = R.gather(A, parity)
    assert set(np.unique(X)) <= set(np.unique(A)) | {0.0}


@pytest.mark.parametrize("parity", R.PARITIES)
def test_the_corpus_holds_what_it_claims(parity):
    """every one of the 12 taps is outside the image at some output position of the corpus and inside at another; (1, 2) has a single
    output per item and every vertical tap outside; (5, 6) has every tap inside somewhere; (9, 30) crosses a wave's 32 positions and a
    block's 128; the channel counts sit on the K-tile, row-tile and row-group edges"""
    outside, inside = np.zeros(12, bool), np.zeros(12, bool)
    for h, w, *_ in R.CORPUS:
        nb = R.neighbours(h, w, parity)
        outside |= (nb < 0).any(1)
        inside |= (nb >= 0).any(1)
    assert outside.all() and inside.all()
    nb = R.neighbours(1, 2, parity)
    assert nb.shape[1] == 1 and all(nb[t, 0] < 0 for t, (i, _) in enumerate(R.TAPS) if i != 2)
    assert (R.neighbours(5, 6, parity) >= 0).any(1).all()
    assert any(h * (w // 2) > 128 for h, w, *_ in R.CORPUS)
    assert {c[2] for c in R.CORPUS} == {1, 2, 31, 32, 33, 65} and {c[3] for c in R.CORPUS} == {1, 31, 32, 33, 193}
    assert {c[4] for c in R.CORPUS} == {1, 3} and {c[:2] for c in R.CORPUS} == {(1, 2), (2, 2), (3, 4), (5, 6), (9, 30)}


def _conv(c_in=4, c_out=8, k=5, **kw):
    conv = torch.nn.Conv2d(c_in, c_out, k, padding=kw.pop("padding", k // 2), **kw)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(R.masked(conv.weight.numpy())) if k == 5 else conv.weight)
    return conv


def test_checkerboard_context_refuses_what_it_cannot_run():
    from flashgmm_amd.ops import CheckerboardContext

    with pytest.raises(RuntimeError):  # a CPU module: no CPU fallback
        CheckerboardContext(_conv())
    with pytest.raises(ValueError):
        CheckerboardContext(_conv(k=3))
    with pytest.raises(ValueError):
        CheckerboardContext(_conv(stride=2))
    with pytest.raises(ValueError):
        CheckerboardContext(_conv(groups=2))
    with pytest.raises(ValueError):
        CheckerboardContext(_conv(), anchor_parity="both")
    bad = _conv()
    with torch.no_grad():
        bad.weight[3, 1, 2, 2] = 1e-30  # the centre tap: dropped by the mask
    with pytest.raises(ValueError):
        CheckerboardContext(bad)
    # ... which a mask buffer takes care of: the effective weight is weight * mask (then the CPU module is refused for being one)
    bad.register_buffer("mask", torch.from_numpy(R.masked(np.ones((8, 4, 5, 5), np.float32))))
    with pytest.raises(RuntimeError):
        CheckerboardContext(bad)
