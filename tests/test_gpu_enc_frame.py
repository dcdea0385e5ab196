"""GPU (-m gpu): the three encode-side CDF kernels held to each other on the same inputs.  symtab_kernel (``compress_batch``),
rate_kernel (``estimate_bits``) and rdoq_kernel (``quantize_rdo``) share one frame (flashgmm_amd/csrc/fgmm_encframe.h): where a wave
sits in the linear and in the tiled grid, how the latent and the twelve planes are loaded per VEC, how a position's mixture is
gathered.  Everything here is exact: bytes, integer sums and float bit patterns, no tolerance.

The matrix kernel x VEC x grid x plane type, and who covers each cell ("own": CASES below, every mode, clamp on and off):

  kernel   VEC  grid    fp32 planes                                     fp16 planes
  symtab   1    tiled   own (12, 7, 9); enc_vec 1 + enc_linear 0 of     own (12, 8, 13) off by one element
                        every own case
  symtab   1    linear  own (6, 8, 8) off by one float; enc_vec 1 of    own (6, 8, 8) off by one element; enc_vec 1 of (4, 16, 32)
                        (16, 16, 16), (6, 8, 8)
  symtab   2    both    own: enc_vec 2 of every case (linear where      own: enc_vec 2 of (12, 8, 13) tiled, (4, 16, 32) both
                        hw % 128 == 0: (16, 16, 16))
  symtab   4    tiled   own (8, 4, 4), (12, 8, 13): a partial wave;     own: enc_vec 4 of (12, 8, 13)
                        enc_linear 0 of (16, 16, 16)
  symtab   4    linear  own (16, 16, 16)                                own: enc_vec 4 of (4, 16, 32)
  symtab   8    tiled   -                                               own (12, 8, 13): a partial wave; enc_linear 0 of (4, 16, 32)
  symtab   8    linear  -                                               own (4, 16, 32)
  rate     1    tiled   own (12, 7, 9): hw = 63, aligned                own (12, 8, 13) off by one element
  rate     1    linear  own (6, 8, 8) off by one float                  own (6, 8, 8) off by one element
  rate     4    tiled   own (8, 4, 4), (12, 8, 13): a partial wave      own (12, 8, 13)
  rate     4    linear  own (16, 16, 16)                                own (4, 16, 32)
  rdoq     1 / 4        as rate, same cases                             as rate, same cases

  The rate / rdoq cell of every own case is ASSERTED (``enc_ref.form_of_one`` on the tensors handed over: CASES' last column); planes with
  hw % 4 != 0 at more sizes, weighted and with channel skipping: tests/test_gpu_enc_forms.py.

  logits:        symtab test_gpu_clamped_edges.py test_compress_batch_every_launch_form / _fp16_launch_forms ("logits"), rate
                 test_gpu_rate.py test_fp16_planes_and_logits_stacked, rdoq test_gpu_rdoq.py test_fp16_planes_and_logits
  from symbols:  symtab only (the raw (n, 4) building block, a null channel list): test_gpu_parity.py and test_gpu_rate.py
                 test_symtab_bits_hip_* through fgmm_build_symtab_hip; no call gives rate_kernel symbols, rdoq_kernel reads y alone
  segmented tables (symtab's row addressing): test_gpu_head.py, test_gpu_clamped_edges.py ("segmented tables")

Every case has half of its channels all-zero (zero_frac 0.5, never all and never none), so the compact channel list matters."""
import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from tests import enc_ref as F
from tests import rate_ref as R
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
SEED = 40  # 0 < coded channels < M at every shape below, clamped or not (asserted)
#         (M, h, w)    fp16   off by one element   rate_kernel's and rdoq_kernel's (vec, linear)
CASES = [((8, 4, 4), False, False, (4, F.TILED)),     # hw 16: 4-wide, tiled, a quarter wave
         ((12, 8, 13), False, False, (4, F.TILED)),   # hw 104 = 4 * 26: 4-wide, tiled, a partial wave
         ((12, 8, 13), True, False, (4, F.TILED)),    # ... fp16: symtab's VEC 8 tiled with a partial wave, the other two 4-wide
         ((12, 8, 13), True, True, (1, F.TILED)),     # ... fp16, off by one element: 1-wide, tiled
         ((12, 7, 9), False, False, (1, F.TILED)),    # hw 63: 1-wide, tiled, every tensor aligned - one lane short of a wave
         ((16, 16, 16), False, False, (4, F.LIN)),    # hw 256: linear, VEC 4
         ((6, 8, 8), False, True, (1, F.LIN)),        # hw 64: 1-wide on the linear grid
         ((6, 8, 8), True, True, (1, F.LIN)),         # ... fp16
         ((4, 16, 32), True, False, (4, F.LIN))]      # hw 512, fp16: symtab VEC 8 linear, the other two VEC 4 linear


def dv(a, off=False):
    """on the device; off: as a dense view one element into its storage (no 16-byte alignment: VEC 1)"""
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    if not off:
        return t
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 != 0
    return out


@pytest.fixture
def enc_options():
    saved = {k: _lib.get_option(0, k) for k in ("enc_vec", "enc_linear")}
    yield lambda **kw: [_lib.set_option(0, k, v) for k, v in kw.items()]
    for k, v in saved.items():
        _lib.set_option(0, k, v)


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_three_kernels_agree_on_the_same_inputs(oracle, enc_options, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for (M, h, w), f16, off, form in CASES:
        name = ((M, h, w), f16, off)
        hw = h * w
        y, s, m, pi = T.make_latent(SEED, M, h, w, clamp=not clamp, zero_frac=0.5)
        planes = T.to_float16_planes(s, m, pi) if f16 else (s, m, pi)
        # ---- the reference, once: the oracle's table of the (widened) planes, priced entry by entry by the host function ---------
        sym, s_, m_, w_, am, zb, _ = T.to_coder_inputs(y, *(a.astype(np.float32) for a in planes), clamp=clamp)
        nz = np.nonzero(zb)[0]
        assert 0 < len(nz) < M, name
        want_bytes = oracle.encode_gmm(mode, sym, s_, m_, w_)
        bits_q, n_byp, cost = R.host_bits(L, oracle.symtab(mode, sym, s_, m_, w_), sym, costs=True)
        chan = np.zeros(M, np.int64)
        chan[nz] = cost.reshape(len(nz), hw).astype(np.int64).sum(1)
        bmap = np.zeros((M, hw), np.float32)
        bmap[nz] = cost.reshape(len(nz), hw).astype(np.float32) * np.float32(2.0 ** -24)
        t = [dv(a, off) for a in (y, *planes)]
        # ---- symtab_kernel: the reference's bytes under every load width and both grids ----------------------------------------
        for vec in (1, 2, 4, 0):
            for linear in (0, 1):
                enc_options(enc_vec=vec, enc_linear=linear)
                (b, am_g, zb_g), _ = gmc.compress_batch(*([a] for a in t))[0]
                assert bytes(b) == want_bytes, (name, vec, linear)
                assert (am_g, zb_g.cpu().tolist()) == (am, zb.tolist()), (name, vec, linear)
        enc_options(enc_vec=0, enc_linear=1)
        # ---- rate_kernel: channel sums and map -----------------------------------------------------------------------------------
        assert F.form_of_one(*t, pos_w=False) == form, name
        est = gmc.estimate_bits(*t, per_channel=True, per_latent=True)
        assert F.form_of_one(*t, pos_w=False, out=est.latent_bits) == form, name
        assert (est.bits_q, est.n_bypass, est.n_symbols) == (bits_q, n_byp, len(sym)), name
        assert (est.abs_max, est.zero_bitmap.tolist()) == (am, zb.tolist()), name
        assert est.channel_bits_q.tolist() == chan.tolist(), name
        assert np.array_equal(est.latent_bits.cpu().numpy().reshape(M, hw).view(np.uint32), bmap.view(np.uint32)), name
        # ---- rdoq_kernel at lambda = 0: round(y), priced as rate_kernel prices it ------------------------------------------------
        q = gmc.quantize_rdo(*t, 0.0, per_channel=True)
        assert F.form_of_one(*t, pos_w=False, out=q.y) == form, name
        want_y = np.round(y) + np.float32(0.0)  # (-0.0 -> +0.0)
        assert np.array_equal(q.y.cpu().numpy().view(np.uint32), want_y.view(np.uint32)), name
        assert q.n_changed == 0 and q.bits_q_before == q.bits_q_after == est.bits_q, name
        assert q.channel_bits_q_after.tolist() == est.channel_bits_q.tolist(), name
