"""GPU (-m gpu): the three decode-side kernel families held to each other on the same item.  tab_kernel (the single-pass tables),
cdftab_count / cdftab_fill (the generic two-pass tables) and segdec_kernel (the segment decoder) share one frame
(flashgmm_amd/csrc/fgmm_decframe.h): the compact channel lookup, a latent's twelve parameters and their way into LDS, the
evaluation window, the row trimming, the evaluation of two consecutive edges, and ONE launch ladder mode x clamp x plane type.
Everything here is exact: symbols and bytes, no tolerance.  A launcher that lands on a neighbouring rung fails, because the item
(tests/dec_frame_items.py) decodes to other symbols under every neighbouring rung: tests/test_dec_frame_cpu.py asserts that on the
CPU oracle, for every case below.

The item: (M, h, w) = (6, 8, 13) - hw = 104, a partial wave and a partial block -, the odd channels dead, sigma on both sides of
the clamp bound, abs_max 44, compressed ONCE per case with checkpoint_stride = 256 - the smallest the library accepts (the entropy
model refuses anything below, and the segment decoder is given nothing below): 312 symbols, one note, two segments.

The matrix kernel family x mode x clamp x plane type, and who runs each rung ("own": test_every_rung_of_the_three_ladders):

  family          modes  clamp     float32                      float16                        bfloat16
  tab_kernel      all 3  on, off   own; test_gpu_parity.py,     own; test_gpu_clamped_edges    own; test_gpu_bf16_planes.py
                                   test_gpu_clamped_edges.py,   .py (fp16 families)            test_decompress*
                                   test_gpu_reference_edges.py
  cdftab_count /  all 3  on, off   own (tab_cap_e = 256);       own (tab_cap_e = 256)          own (tab_cap_e = 256);
  cdftab_fill                      the "generic" legs of the                                   test_gpu_bf16_planes.py "wide"
                                   files above
  segdec_kernel   all 3  on, off   own (gpu_decode = 1);        own; test_gpu_segdec_edges.py  own; test_gpu_bf16_planes.py
                                   test_gpu_segdec_edges.py     test_fp16_planes_and_...       test_segment_decoder_settles_...

  logits:            test_gpu_parity.py (decode from logits, both table kernels), test_gpu_clamped_edges.py ("logits")
  8-byte headers:    test_gpu_parity.py (max_bs past 16382, the generic kernels)
  2-byte headers and their escape, Elias-Fano rows: test_gpu_parity.py, test_gpu_symbol_sweep.py

Which kernel decoded is asserted, not assumed: the single-pass kernel counts its edges (ctx_stat 3 > 0), the generic kernels do not
(== 0), and the segment decoder must settle the item itself ((ctx_stat 4, ctx_stat 5) == (1, 0)): the table path would take over
- and hide - a segment that fails its note."""
import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, _lib
from tests import dec_frame_items as D

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dv(a, kind="float32"):
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if kind == "bfloat16" else np.ascontiguousarray(a)).to(DEV)
    return t.view(torch.bfloat16) if kind == "bfloat16" else t


@pytest.fixture
def ctx_options():
    """set options of the process-wide context for one test and restore them afterwards (gpu_decode back to 0, profiling off)"""
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, _lib.get_option(0, k))
            _lib.set_option(0, k, v)

    try:
        yield set_
    finally:
        for k, v in saved.items():
            _lib.set_option(0, k, v)
        _lib.set_option(0, "gpu_decode", 0)
        _lib.set_profiling(0, False)


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", D.MODES)
@pytest.mark.parametrize("kind", D.PLANES)
def test_every_rung_of_the_three_ladders(oracle, ctx_options, kind, mode, clamp):
    name = f"{kind} {mode} clamp={clamp}"
    y = dv(D.make_item()[0])
    p = [dv(a, kind) for a in D.planes(kind)[0]]
    assert p[0].dtype == getattr(torch, kind)
    sym, rows, am, zb, yq = D.coded(kind, clamp)
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp, checkpoint_stride=D.STRIDE)
    (b, am_g, zb_g), yq_g = gmc.compress_batch([y], *([a] for a in p))[0]
    assert isinstance(b, CheckpointedBytes) and len(b.ckpt) == (len(sym) - 1) // D.STRIDE == 1, name
    assert (am_g, zb_g.cpu().tolist()) == (am, zb.tolist()), name
    assert np.array_equal(yq_g.cpu().numpy(), yq), name
    if kind == "float32":
        assert bytes(b) == oracle.encode_gmm(mode, sym, *rows), name
    want = torch.from_numpy(yq).to(DEV)

    def decode(stream):
        return gmc.decompress_batch([stream], [am_g], [zb_g], *([a] for a in p))[0]

    cap0 = _lib.get_option(0, "tab_cap_e")
    _lib.set_profiling(0, True)  # (the single-pass kernel counts its edges only then)
    # ---- tab_kernel: the plain stream (no notes: nothing but the table path can take it), default options ---------------------
    ctx_options(gpu_decode=0, tab_cap_e=cap0)
    got = decode(bytes(b))
    assert _lib.ctx_stat(0, 3) > 0, f"{name}: the single-pass kernel did not run"
    assert torch.equal(got, want), f"{name}: tab_kernel"
    # ---- cdftab_count / cdftab_fill: an LDS budget no latent of the item fits ----------------------------------------------------
    ctx_options(tab_cap_e=256)
    got = decode(bytes(b))
    assert _lib.ctx_stat(0, 3) == 0, f"{name}: the generic kernels did not run"
    assert torch.equal(got, want), f"{name}: cdftab_count / cdftab_fill"
    # ---- segdec_kernel: the stream with its notes, decoded on the GPU and settled there ----------------------------------------
    ctx_options(tab_cap_e=cap0, gpu_decode=1)
    got = decode(b)
    assert (_lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5)) == (1, 0), f"{name}: (settled by the segment decoder, handed back)"
    assert torch.equal(got, want), f"{name}: segdec_kernel"
