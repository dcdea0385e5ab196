"""GPU (-m gpu): the coded size without running the coder (include/flashgmm_amd.h section 3b) - fgmm_symtab_bits_hip against the
host's fgmm_symtab_bits, ``estimate_bits_batch`` (rate_kernel, flashgmm_amd/csrc/fgmm_rate.hip) against the oracle's tables priced by
the host function and against the lengths of the streams the oracle's encoder and ``compress`` write.

Which streams may miss the predicted length by 4 bytes is decided by tests/rate_ref.py left_out (float64 B within 0.05 bit of a
multiple of 32), from the oracle's table alone; a test fails when more than one stream in ten is left out."""
import ctypes as C

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, RateEstimate, _lib
from tests import edge_corpus as E
from tests import enc_ref as F
from tests import rate_ref as R
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_bits(packed, symbols=None):
    """fgmm_symtab_bits_hip -> (bits_q, n_bypass, cost_q uint32[n])"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    p = packed if isinstance(packed, torch.Tensor) else dv(np.asarray(packed, np.uint32).view(np.int32))
    n = p.numel()
    s = None if symbols is None else (symbols if isinstance(symbols, torch.Tensor) else dv(np.asarray(symbols, np.int32)))
    cost = torch.full((max(n, 1),), -1, dtype=torch.int32, device=DEV)
    tot = torch.full((2,), 77, dtype=torch.int64, device=DEV)  # (overwritten, not added to)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_symtab_bits_hip(ctx, None, p.data_ptr(), s.data_ptr() if s is not None else None, n, cost.data_ptr(), tot.data_ptr(),
                                      tot.data_ptr() + 8))
    t = tot.cpu().tolist()
    return t[0], t[1], cost[:n].cpu().numpy().view(np.uint32)


def gpu_symtab(mode, v, s, m, w):
    """fgmm_build_symtab_hip on (n, 4) rows -> device int32[n]"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    v, s, m, w = dv(v.astype(np.int32)), dv(s), dv(m), dv(w)
    out = torch.empty(v.numel(), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_build_symtab_hip(ctx, None, v.data_ptr(), s.data_ptr(), m.data_ptr(), w.data_ptr(), v.numel(), s.stride(0), s.stride(1),
                                       _lib.mode_id(mode), out.data_ptr()))
    return v, out


def reference(oracle, mode, y, s, m, w, clamp):
    """what an estimate of (y, s, m, w) must say, from the oracle's table priced by the host function"""
    L = _lib.lib()
    M, hw = y.shape[1], y.shape[2] * y.shape[3]
    sym, s_, m_, w_, am, zb, _ = T.to_coder_inputs(y, s, m, w, clamp=clamp)
    ref = {"abs_max": am, "zero_bitmap": zb.tolist(), "n_symbols": len(sym), "chan": np.zeros(M, np.int64), "map": np.zeros((M, hw), np.float32)}
    if len(sym) == 0:
        ref.update(bits_q=0, n_bypass=0, true_len=8, b64=0.0)
        return ref
    packed = oracle.symtab(mode, sym, s_, m_, w_)
    bits_q, nb, cost = R.host_bits(L, packed, sym, costs=True)
    nz = np.nonzero(zb)[0]
    ref["chan"][nz] = cost.reshape(len(nz), hw).astype(np.int64).sum(1)
    ref["map"][nz] = cost.reshape(len(nz), hw).astype(np.float32) * np.float32(2.0 ** -24)
    ref.update(bits_q=bits_q, n_bypass=nb, true_len=len(oracle.encode_gmm(mode, sym, s_, m_, w_)), b64=R.float_bits(packed, sym))
    return ref


def check(est, ref, tally, name):
    assert isinstance(est, RateEstimate)
    assert (est.abs_max, est.zero_bitmap.tolist(), est.n_symbols) == (ref["abs_max"], ref["zero_bitmap"], ref["n_symbols"]), name
    assert (est.bits_q, est.n_bypass) == (ref["bits_q"], ref["n_bypass"]), name
    assert est.bits == ref["bits_q"] / R.ONE and est.nbytes == _lib.lib().fgmm_rate_stream_bytes(est.bits_q)
    if est.channel_bits_q is not None:
        assert est.channel_bits_q.tolist() == ref["chan"].tolist(), name
        assert est.channel_bits.tolist() == (ref["chan"] / R.ONE).tolist()
    if est.latent_bits is not None:
        got = est.latent_bits.cpu().numpy()
        assert got.shape[:2] == (1, len(ref["chan"])) and np.array_equal(got.reshape(ref["map"].shape).view(np.uint32), ref["map"].view(np.uint32)), name
    tally[0] += 1
    if R.left_out(ref["b64"]):
        tally[1] += 1
        assert abs(est.nbytes - ref["true_len"]) <= 4, name
    else:
        assert est.nbytes == ref["true_len"], (name, est.nbytes, ref["true_len"], ref["b64"])


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def test_symtab_bits_hip_equals_the_host_function():
    """per entry and in total: every range 1 .. 65535 and the bypass list; 1, 63, 64, 65 and 257 entries (the wave's and the block's
    edges); with the symbols and without (then a bypass entry is priced by its low half, sign-extended)"""
    L = _lib.lib()
    r = np.arange(1, 65536, dtype=np.uint32)
    byp = np.array(R.BYPASS_SYMBOLS, np.int64).astype(np.int32)
    packed = np.concatenate([r << 16, byp.view(np.uint32) & 0xFFFF]).astype(np.uint32)
    sym = np.concatenate([np.zeros(len(r), np.int32), byp])
    want = R.host_bits(L, packed, sym, costs=True)
    got = gpu_bits(packed, sym)
    assert got[:2] == want[:2] and np.array_equal(got[2], want[2])
    assert (got[2][len(r):].astype(np.int64) // R.ONE).tolist() == R.BYPASS_BITS and got[1] == len(byp)
    want0 = R.host_bits(L, packed, None, costs=True)
    got0 = gpu_bits(packed, None)
    assert got0[:2] == want0[:2] and np.array_equal(got0[2], want0[2]) and want0[0] != want[0]
    rng = np.random.default_rng(5)
    pick = rng.permutation(len(packed))
    for n in (0, 1, 63, 64, 65, 257):
        p, s = packed[pick[:n]], sym[pick[:n]]
        p[: min(n, 2)] = byp.view(np.uint32)[5:5 + min(n, 2)] & 0xFFFF  # a bypass entry in the first wave whatever n is
        s[: min(n, 2)] = byp[5:5 + min(n, 2)]
        want = R.host_bits(L, p, s, costs=True)
        got = gpu_bits(p, s)
        assert got[:2] == want[:2] and np.array_equal(got[2], want[2]), n


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
SHAPES = [(8, 4, 4),     # hw = 16: a quarter of a wave, the 4-wide loads
          (32, 16, 8),   # hw = 128: 4-wide, half a block per channel
          (12, 8, 13),   # hw = 104 = 4 * 26: 4-wide too, tiled, a partial wave (planes with hw % 4 != 0: tests/test_gpu_enc_forms.py)
          (16, 16, 16)]  # hw = 256 = 64 * 4: the linear grid
FORMS = [(4, F.TILED), (4, F.TILED), (4, F.TILED), (4, F.LIN)]  # the launch form of a batch of each shape, asserted on the call's tensors


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_estimate_bits_batch_against_the_oracle(oracle, mode, clamp):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    tally = [0, 0]
    for shape, form in zip(SHAPES, FORMS):
        cases = [T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf) for seed, zf in ((3, 0.0), (4, 0.5), (5, 0.0), (6, 0.5))]
        cols = [[dv(a) for a in col] for col in zip(*cases)]
        assert F.form_of(*cols) == form, shape
        est = gmc.estimate_bits_batch(*cols, per_channel=True, per_latent=True)
        assert F.form_of(*cols, outs=[e.latent_bits for e in est]) == form, shape
        assert len(est) == len(cases)
        for i, (e, c) in enumerate(zip(est, cases)):
            check(e, reference(oracle, mode, *c, clamp), tally, (shape, i))
        plain = gmc.estimate_bits_batch(*([dv(a) for a in col] for col in zip(*cases)))  # (no map, no channel sums asked for)
        assert [(p.bits_q, p.nbytes, p.channel_bits_q, p.latent_bits) for p in plain] == [(e.bits_q, e.nbytes, None, None) for e in est]
    # every channel all-zero: nothing is coded - the empty stream
    y, s, m, w = T.make_latent(7, 8, 4, 4, clamp=not clamp)
    e = gmc.estimate_bits(dv(np.zeros_like(y)), dv(s), dv(m), dv(w), per_channel=True, per_latent=True)
    check(e, reference(oracle, mode, np.zeros_like(y), s, m, w, clamp), tally, "all zero")
    assert (e.bits_q, e.nbytes, e.n_symbols, e.abs_max, int(e.zero_bitmap.sum())) == (0, 8, 0, 1, 0) and not e.latent_bits.any()
    # hw = 64 at an address that is not 16-byte aligned: the 1-wide path on the linear grid
    y, s, m, w = T.make_latent(8, 4, 8, 8, clamp=not clamp, zero_frac=0.3)
    buf = torch.zeros(y.size + 1, dtype=torch.float32, device=DEV)
    buf[1:] = dv(y).reshape(-1)
    t = (buf[1:].view(1, 4, 8, 8), dv(s), dv(m), dv(w))
    assert F.form_of_one(*t, pos_w=False) == (1, F.LIN)
    e = gmc.estimate_bits(*t, per_channel=True, per_latent=True)
    check(e, reference(oracle, mode, y, s, m, w, clamp), tally, "misaligned")
    assert tally[1] * 10 <= tally[0], tally


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fp16_planes_and_logits_stacked(mode):
    """stacked calls: float16 planes, and float32 planes with the weights given as logits - bits_q is the cost of the table
    fgmm_build_symtab_hip builds from the widened / soft-maxed parameters, nbytes the length of compress_batch's bitstream"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    cases = [T.make_latent(20 + i, 32, 16, 8, clamp=False, zero_frac=0.2) for i in range(3)]
    ys = np.concatenate([c[0] for c in cases])
    # float16 planes
    p16 = [T.to_float16_planes(*c[1:]) for c in cases]
    planes = [dv(np.concatenate([p[k] for p in p16])) for k in range(3)]
    est = gmc.estimate_bits_batch(dv(ys), *planes, per_channel=True)
    enc = gmc.compress_batch(dv(ys), *planes)
    for i, (c, p) in enumerate(zip(cases, p16)):
        sym, s_, m_, w_, am, zb, _ = T.to_coder_inputs(c[0], *(a.astype(np.float32) for a in p))
        vd, tab = gpu_symtab(mode, sym, s_, m_, w_)
        bits_q, nb, cost = gpu_bits(tab, vd)
        assert (est[i].bits_q, est[i].n_bypass, est[i].n_symbols, est[i].abs_max) == (bits_q, nb, len(sym), am), i
        assert est[i].zero_bitmap.tolist() == zb.tolist() == enc[i][0][2].tolist() and est[i].abs_max == enc[i][0][1]
        assert est[i].channel_bits_q[torch.from_numpy(zb != 0)].tolist() == cost.reshape(int(zb.sum()), -1).astype(np.int64).sum(1).tolist()
        assert est[i].nbytes == len(enc[i][0][0]), (i, est[i].nbytes, len(enc[i][0][0]), est[i].bits)
    # logits
    lgs = [np.log(c[3]).astype(np.float32) for c in cases]
    planes = [dv(np.concatenate([c[1] for c in cases])), dv(np.concatenate([c[2] for c in cases])), dv(np.concatenate(lgs))]
    est = gmc.estimate_bits_batch(dv(ys), *planes, weights_are_logits=True)
    enc = gmc.compress_batch(dv(ys), *planes, weights_are_logits=True)
    for i, (c, lg) in enumerate(zip(cases, lgs)):
        sym, s_, m_, lg_, am, zb, _ = T.to_coder_inputs(c[0], c[1], c[2], lg)
        lg_d = dv(lg_)
        pi_d = torch.empty_like(lg_d)
        torch.cuda.synchronize()
        _lib.check(L.fgmm_softmax4_hip(ctx, None, lg_d.data_ptr(), pi_d.data_ptr(), len(sym)))
        vd, tab = gpu_symtab(mode, sym, s_, m_, pi_d.cpu().numpy())
        bits_q, nb, _ = gpu_bits(tab, vd)
        assert (est[i].bits_q, est[i].n_bypass, est[i].n_symbols) == (bits_q, nb, len(sym)), i
        assert est[i].nbytes == len(enc[i][0][0]), (i, est[i].nbytes, len(enc[i][0][0]), est[i].bits)


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_edge_latents(oracle, mode):
    """every family of edge_corpus.latent_case - NaN, +-inf, beyond int32, ties, -0.0, abs_max at the symbol width's edges: the side
    information is compress's, the predicted length within 4 bytes of its bitstream and equal to it outside the left-out streams"""
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    fams = list(E.LATENT_FAMILIES)
    cases = [E.latent_case(f) for f in fams]
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    enc = gmc.compress_batch(*cols)
    est = gmc.estimate_bits_batch(*cols)
    assert len(est) == len(enc) == len(fams)
    n_left = 0
    for f, c, e, ((b, am, zb), _) in zip(fams, cases, est, enc):
        assert (e.abs_max, e.zero_bitmap.tolist()) == (am, zb.tolist()), f
        assert e.n_symbols == int(zb.sum()) * c[0].shape[2] * c[0].shape[3], f
        assert abs(e.nbytes - len(b)) <= 4, (f, e.nbytes, len(b))
        sym, s_, m_, w_, *_ = T.to_coder_inputs(*c)
        packed = oracle.symtab(mode, sym, s_, m_, w_)
        assert (e.bits_q, e.n_bypass) == R.host_bits(_lib.lib(), packed, sym), f
        if R.left_out(R.float_bits(packed, sym)):
            n_left += 1
        else:
            assert e.nbytes == len(b), (f, e.nbytes, len(b), e.bits)
    assert n_left * 10 <= len(fams), n_left


# ---- (e) ------------------------------------------------------------------------------------------------------------------------
def test_mixed_shapes_and_determinism():
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    shapes = [(8, 4, 4), (12, 8, 13), (16, 16, 16), (32, 16, 8), (5, 3, 7)]
    cases = [[dv(a) for a in T.make_latent(40 + i, *shp, clamp=False, zero_frac=0.3)] for i, shp in enumerate(shapes)]
    cols = [list(col) for col in zip(*cases)]
    key = lambda e: (e.bits_q, e.nbytes, e.n_symbols, e.n_bypass, e.abs_max, e.zero_bitmap.tolist(), e.channel_bits_q.tolist(),  # noqa: E731
                     e.latent_bits.cpu().numpy().tobytes())
    batch = gmc.estimate_bits_batch(*cols, per_channel=True, per_latent=True)
    singles = [gmc.estimate_bits(*c, per_channel=True, per_latent=True) for c in cases]
    assert [key(e) for e in batch] == [key(e) for e in singles]
    assert all(e.bits_q > 0 for e in batch)
    again = gmc.estimate_bits_batch(*cols, per_channel=True, per_latent=True)
    assert [key(e) for e in again] == [key(e) for e in batch]


# ---- (f) ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_checkerboard_estimate_equals_the_bitstreams_lengths(mode):
    """CheckerboardLatentCodec.estimate on the exact networks of tests/synth.py, at the sizes of the codec parity test's checkerboard
    cases (tests/golden/make_golden.py G7_CKBD): each half's nbytes is the length of that half's bitstream"""
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    Ctx, Par = T.exact_modules()
    for seed, c, c_side, h, w, dead, quantizer, parity in ((11, 6, 8, 8, 12, 0, "noise", "even"), (12, 5, 6, 6, 10, 1, "weighted_mean_ste", "odd")):
        y, side = T.exact_codec_inputs(seed, c, c_side, h, w, dead=dead)
        codec = CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode=mode)},
                                        context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c), anchor_parity=parity).cuda()
        enc = codec.compress(dv(y), dv(side))
        got = codec.estimate(dv(y), dv(side))
        assert [e.nbytes for e in got["estimates"]] == [len(b) for b, _, _ in enc["strings"]], (seed, [e.bits for e in got["estimates"]])
        assert [(e.abs_max, e.zero_bitmap.tolist()) for e in got["estimates"]] == [(a, zb.tolist()) for _, a, zb in enc["strings"]]
        assert got["nbytes"] == sum(len(b) for b, _, _ in enc["strings"]) and got["bits_q"] == sum(e.bits_q for e in got["estimates"])
        assert got["bits"] == got["bits_q"] / R.ONE
