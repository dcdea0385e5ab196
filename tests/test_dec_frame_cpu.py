"""No GPU: the item of tests/test_gpu_dec_frame.py (tests/dec_frame_items.py) DISCRIMINATES the rungs of the decode-side launch
ladder.  The GPU test asserts equality with the coded symbols and no tolerance; that only pins a rung if the neighbouring rungs give
something else.  So for every plane type, mode and clamp flag, the CPU oracle's decoder, run on the item's own stream with

  * each of the two other modes, and
  * the clamp flipped at the same mode,

must not return the coded symbols (it returns other symbols, or refuses a stream that has lost its meaning).  Polya against
Abramowitz & Stegun is the close pair: their tables differ in few edges."""
import numpy as np
import pytest

from tests import dec_frame_items as D


def _decoded(oracle, mode, data, rows, am):
    try:
        return oracle.decode_gmm(mode, data, *rows, am + 1)
    except RuntimeError:
        return None  # the stream ran out under the wrong model


def test_item_is_what_the_gpu_test_says_it_is():
    M, h, w = D.SHAPE
    y, sg, _, _ = D.make_item()
    for kind in D.PLANES:
        for clamp in (True, False):
            sym, _, am, zb, _ = D.coded(kind, clamp)
            assert zb.tolist() == [1, 0] * (M // 2)           # half the channels dead, in between the coded ones
            assert D.STRIDE < len(sym) == (M // 2) * h * w    # at least one note: the segment decoder takes the item
            assert 10 <= am < 100                             # a few tens: 2 * (am + 1) + 2 edges fit every decode-side kernel
        s_live = D.planes(kind)[1][0].reshape(4, M, h * w)[:, ::2]
        assert (s_live < np.float32(0.11)).mean() > 0.02 and (s_live > np.float32(0.11)).mean() > 0.5  # both sides of the clamp bound


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("kind", D.PLANES)
def test_neighbouring_rungs_decode_other_symbols(oracle, kind, mode, clamp):
    sym, rows, am, _, _ = D.coded(kind, clamp)
    data = oracle.encode_gmm(mode, sym, *rows)
    assert np.array_equal(oracle.decode_gmm(mode, data, *rows, am + 1), sym)  # the rung itself
    for other in D.MODES:
        if other != mode:
            got = _decoded(oracle, other, data, rows, am)
            assert got is None or not np.array_equal(got, sym), f"{kind} {mode} clamp={clamp}: mode {other} decodes the same symbols"
    flipped = D.coded(kind, not clamp)[1]
    got = _decoded(oracle, mode, data, flipped, am)
    assert got is None or not np.array_equal(got, sym), f"{kind} {mode} clamp={clamp}: the flipped clamp decodes the same symbols"
