"""GPU (-m gpu): rate-distortion optimised quantisation (include/flashgmm_amd.h section 3c; rdoq_kernel,
flashgmm_amd/csrc/fgmm_rdoq.hip) against tests/rdoq_ref.py - the oracle's tables for the symbols sym - 1, sym, sym + 1 priced by the
host's fgmm_symtab_bits, the objective in float64.  Every output is compared for EQUALITY: the chosen latents bit for bit, the counts
and the integer sums.  The conditions that keep the sweep from passing vacuously (at lambda = 0.5 at least 5 % of the coded latents
move in every case; some move goes away from zero; some candidate is priced as a bypass escape) hold for every mode, clamped and not,
with seeds 3 and 4: tests/test_rdoq_cpu.py checks them on the CPU, the sweep below asserts them again."""
import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, RdoQuantized, _lib
from tests import edge_corpus as E
from tests import enc_ref as F
from tests import rate_ref as R
from tests import rdoq_ref as Q
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(got, ref, name):
    assert isinstance(got, RdoQuantized)
    y = got.y.cpu().numpy()
    assert Q.same_float_bits(y, ref["y"]), (name, int((y.view(np.uint32) != ref["y"].view(np.uint32)).sum()))
    assert (got.n_changed, got.bits_q_before, got.bits_q_after) == (ref["n_changed"], ref["bits_q_before"], ref["bits_q_after"]), name
    assert (got.abs_max, got.zero_bitmap.tolist()) == (ref["abs_max"], ref["zero_bitmap"]), name
    assert got.bits_before == ref["bits_q_before"] / R.ONE and got.bits_after == ref["bits_q_after"] / R.ONE
    if got.channel_bits_q_after is not None:
        assert got.channel_bits_q_after.tolist() == ref["chan_after"].tolist(), name


def key(q):
    return (q.y.cpu().numpy().tobytes(), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, q.zero_bitmap.tolist(),
            None if q.channel_bits_q_after is None else q.channel_bits_q_after.tolist())


# ---- (a) the main sweep -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_quantize_rdo_against_the_reference(oracle, mode, clamp):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    cases = [T.make_latent(seed, *shape, clamp=not clamp, zero_frac=zf) for shape in Q.SHAPES for seed, zf in Q.SEEDS]
    cols = [[dv(a) for a in col] for col in zip(*cases)]
    away = byp = 0
    for lam in Q.LAMBDAS:
        refs = [Q.rdoq(oracle, L, mode, *c, lam, clamp=clamp) for c in cases]
        assert F.form_of(*cols) == (4, F.TILED)  # mixed shapes, every hw a multiple of 4: 4-wide on the tiled grid
        got = gmc.quantize_rdo_batch(*cols, lam, per_channel=True)
        assert len(got) == len(cases)
        for i, (g, r) in enumerate(zip(got, refs)):
            check(g, r, (lam, i))
            away += r["n_away"]
            byp += r["n_bypass_cand"]
            if lam == 0.5:
                assert r["n_changed"] * 20 >= r["n_coded"] > 0, (i, r["n_changed"], r["n_coded"])
            if lam == 0.0:
                assert g.n_changed == 0 and g.bits_q_after == g.bits_q_before
        # single calls (each shape on its own grid: 4-wide, tiled at hw = 16, 128 and 104, linear at 256) agree with the batch; without
        # the channel sums too
        assert [F.form_of_one(*(col[i] for col in cols), pos_w=False) for i in range(0, len(cases), 2)] == [(4, F.TILED)] * 3 + [(4, F.LIN)]
        singles = [gmc.quantize_rdo(*(col[i] for col in cols), lam, per_channel=True) for i in range(len(cases))]
        assert [key(s) for s in singles] == [key(g) for g in got], lam
        for s, r in zip(singles, refs):
            check(s, r, (lam, "single"))
        plain = gmc.quantize_rdo(*(col[1] for col in cols), lam)
        assert plain.channel_bits_q_after is None and key(plain)[:-1] == key(got[1])[:-1]
        # stacked tensors: the two seeds of one shape as [2, ...] tensors
        for k in range(len(Q.SHAPES)):
            st = gmc.quantize_rdo_batch(*(torch.cat(col[2 * k:2 * k + 2]) for col in cols), lam, per_channel=True)
            assert [key(s) for s in st] == [key(g) for g in got[2 * k:2 * k + 2]], (lam, k)
    assert away > 0 and byp > 0, (away, byp)
    again = gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True)  # the same bits on every run
    assert [key(a) for a in again] == [key(g) for g in gmc.quantize_rdo_batch(*cols, 0.5, per_channel=True)]


# ---- (b) end to end ---------------------------------------------------------------------------------------------------------------
def lone_one_case(seed=11):
    """a latent whose channel 1 has ONE non-zero round(y), a +1 of low probability (a narrow mixture at 0): at lambda = 0.5 RDOQ moves it
    to 0 and the whole channel is no longer coded; channel 2 the same with a lone -1"""
    y, s, m, w = T.make_latent(seed, 8, 4, 4)
    M, hw = 8, 16
    s, m = s.copy().reshape(4, M, hw), m.copy().reshape(4, M, hw)
    y = y.copy()
    for c, v in ((1, 0.6), (2, -0.7)):
        y[0, c] = 0.0
        y[0, c].reshape(-1)[5] = v
        s[:, c], m[:, c] = 0.11, 0.0
    return y, s.reshape(1, 4 * M, 4, 4), m.reshape(1, 4 * M, 4, 4), w


@pytest.mark.parametrize("mode", MODES)
def test_end_to_end_bytes_decode_and_size(oracle, mode):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    cases = [T.make_latent(seed, *shape, clamp=False, zero_frac=zf) for shape in Q.SHAPES for seed, zf in Q.SEEDS] + [lone_one_case()]
    n_left = 0
    for i, c in enumerate(cases):
        t = [dv(a) for a in c]
        ref = Q.rdoq(oracle, L, mode, *c, 0.5)
        q = gmc.quantize_rdo(*t, 0.5)
        check(q, ref, i)
        if i == len(cases) - 1:  # the lone +-1 went to zero and took its channel out of the stream
            zb0 = T.to_coder_inputs(*c)[5]
            assert zb0[1] == 1 and zb0[2] == 1 and ref["zero_bitmap"][1] == 0 and ref["zero_bitmap"][2] == 0 and not ref["y"][0, 1:3].any()
        sym, s_, m_, w_, am, zb, _ = T.to_coder_inputs(ref["y"], *c[1:])  # the channels coded for y_rdo
        want = oracle.encode_gmm(mode, sym, s_, m_, w_)
        (b, am_g, zb_g), yq = gmc.compress(q.y, *t[1:])
        assert bytes(b) == want, i
        assert (am_g, zb_g.cpu().tolist()) == (am, zb.tolist()) == (q.abs_max, q.zero_bitmap.tolist())
        assert torch.equal(yq, q.y) and torch.equal(gmc.decompress(b, am_g, zb_g, *t[1:]), q.y), i
        est = gmc.estimate_bits(q.y, *t[1:])
        packed = oracle.symtab(mode, sym, s_, m_, w_) if len(sym) else np.zeros(0, np.uint32)
        if R.left_out(R.float_bits(packed, sym)):
            n_left += 1
            assert abs(est.nbytes - len(want)) <= 4, i
        else:
            assert est.nbytes == len(want), (i, est.nbytes, len(want))
    assert n_left * 10 <= len(cases), n_left


# ---- (c) fp16 planes, logits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fp16_planes_and_logits(oracle, mode):
    L, ctx = _lib.lib(), _lib.ctx(0)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    y, s, m, w = T.make_latent(21, 32, 16, 8, clamp=False, zero_frac=0.2)
    p16 = T.to_float16_planes(s, m, w)
    for lam in (0.1, 0.5):
        ref = Q.rdoq(oracle, L, mode, y, *(a.astype(np.float32) for a in p16), lam)  # the widened planes
        check(gmc.quantize_rdo(dv(y), *(dv(a) for a in p16), lam, per_channel=True), ref, ("fp16", lam))
        assert ref["n_changed"] > 0
    # logits: the reference gets the weights the kernels' own softmax over K makes of them (fgmm_softmax4_hip, rows (n, 4))
    M, hw = 32, 128
    lg = np.log(w).astype(np.float32)
    rows = dv(lg.reshape(4, M * hw).T)
    pi_d = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), pi_d.data_ptr(), M * hw))
    pi = np.ascontiguousarray(pi_d.cpu().numpy().T).reshape(1, 4 * M, 16, 8)
    for lam in (0.1, 0.5):
        ref = Q.rdoq(oracle, L, mode, y, s, m, pi, lam)
        check(gmc.quantize_rdo(dv(y), dv(s), dv(m), dv(lg), lam, weights_are_logits=True, per_channel=True), ref, ("logits", lam))


# ---- (d) edges ------------------------------------------------------------------------------------------------------------------------
def edge_latents():
    """NaN, +-inf, |round(y)| = 2^20 (considered) and 2^20 + 1 (left alone), exact halves, latents beyond int32 - each with a mixture
    component at the latent itself, so that the neighbours' costs differ"""
    M, h, w = 12, 8, 16
    y, s, m, p = E.latent_case("ties_half", M, h, w)
    y, s, m = y.copy(), s.copy().reshape(4, -1), m.copy().reshape(4, -1)
    vals = [np.nan, np.inf, -np.inf, 2.0 ** 20, -(2.0 ** 20), 2.0 ** 20 + 0.25, 2.0 ** 20 - 0.25, 2.0 ** 20 + 1, -(2.0 ** 20) - 1, 2.0 ** 20 + 0.75,
            0.5, -2.5, 1.5, -0.5, 3e9, -2147483904.0, 2.0 ** 24 + 2]
    rng = np.random.default_rng(9)
    at = rng.choice(y.size, len(vals), replace=False)
    flat = y.reshape(-1)
    for a, v in zip(at, vals):
        flat[a] = np.float32(v)
        if np.isfinite(v):
            m[0, a] = np.float32(v) + np.float32(0.4)
            m[1, a] = np.float32(v) - np.float32(1.2)
            s[:2, a] = np.float32(0.7)
    return (y, s.reshape(1, 4 * M, h, w), m.reshape(1, 4 * M, h, w), p), at, vals


@pytest.mark.parametrize("mode", MODES)
def test_edge_latents(oracle, mode):
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    case, at, vals = edge_latents()
    t = [dv(a) for a in case]
    for lam in (0.0, 0.5, 5.0):
        ref = Q.rdoq(oracle, L, mode, *case, lam)
        q = gmc.quantize_rdo(*t, lam, per_channel=True)
        check(q, ref, ("edges", lam))
        out = q.y.cpu().numpy().reshape(-1)
        for a, v in zip(at, vals):  # NaN, +-inf and everything beyond 2^20 keep round(y)
            if not np.isfinite(v) or abs(np.round(np.float32(v))) > 2.0 ** 20:
                assert Q.same_float_bits(out[a], np.round(np.float32(v))), (lam, v)
    # at lambda = 5 the latents AT +-2^20 are considered: the reference moves at least one of them (towards the component at v + 0.4 / v - 1.2)
    ref = Q.rdoq(oracle, L, mode, *case, 5.0)
    moved = [v for a, v in zip(at, vals) if np.isfinite(v) and abs(np.round(np.float32(v))) == 2.0 ** 20 and
             ref["y"].reshape(-1)[a] != np.round(np.float32(v))]
    assert moved, "no latent at |round(y)| = 2^20 moves: the edge case shows nothing"
    # the other latent families: the same equality
    for fam in ("neg_zero", "one_nan", "beyond_int32_mean_there", "abs_max_32768"):
        c = E.latent_case(fam)
        check(gmc.quantize_rdo(*(dv(a) for a in c), 0.5, per_channel=True), Q.rdoq(oracle, L, mode, *c, 0.5), fam)


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_edge_parameters(oracle, mode, clamp):
    """rows of tests/edge_corpus.py PARAM_FAMILIES as planes - negative, zero, non-finite, tiny and huge sigma, far-off and non-finite
    means: un-clamped they go through the IEEE evaluation, clamped through the guards of the packed fast path (edge by edge)"""
    L = _lib.lib()
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    M, h, w = 6, 8, 13  # hw = 104 and, below, 8 x 16: both 4-wide, tiled - 26 lanes of one wave, and two full waves
    for fam in ("neg_sigma", "zero_sigma", "nonfinite_sigma", "tiny_and_huge_sigma", "huge_mu", "nonfinite_mu", "wide_sigma"):
        for (hh, ww) in ((h, w), (8, 16)):
            n = M * hh * ww
            p = E.param_case(fam, n)
            rng = np.random.default_rng(3)
            y = (np.clip(p["v"], -60, 60) + rng.uniform(-0.5, 0.5, n)).astype(np.float32).reshape(1, M, hh, ww)
            planes = [np.ascontiguousarray(p[k].reshape(M, hh, ww, 4).transpose(3, 0, 1, 2).reshape(1, 4 * M, hh, ww)) for k in ("s", "m", "w")]
            ref = Q.rdoq(oracle, L, mode, y, *planes, 0.5, clamp=clamp)
            t = [dv(y)] + [dv(a) for a in planes]
            assert F.form_of_one(*t, pos_w=False) == (4, F.TILED)
            check(gmc.quantize_rdo(*t, 0.5, per_channel=True), ref, (fam, hh, ww))


# ---- (e) arguments ----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_and_all_zero():
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    y, s, m, w = (dv(a) for a in T.make_latent(7, 8, 4, 4))
    for lam in (-0.5, float("nan"), float("inf")):
        with pytest.raises((ValueError, RuntimeError)):
            gmc.quantize_rdo(y, s, m, w, lam)
        # the C entry point itself refuses it
        it = _lib.fgmm_rdoq_item()
        assert _lib.lib().fgmm_gmc_rdoq_batch(_lib.ctx(0), None, it, 1, 0, 1, lam) == 1
    with pytest.raises(RuntimeError):
        GaussianMixtureConditional(K=3, mode="polya").quantize_rdo(y, s[:, :24], m[:, :24], w[:, :24], 0.5)
    it = _lib.fgmm_rdoq_item()
    it.K, it.M, it.hw = 3, 0, 0
    assert _lib.lib().fgmm_gmc_rdoq_batch(_lib.ctx(0), None, it, 1, 0, 1, 0.5) == 1  # K != 4
    # all-zero y: all zeros, zero sums
    q = gmc.quantize_rdo(torch.zeros_like(y) - 0.0, s, m, w, 0.5, per_channel=True)
    assert (q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, int(q.zero_bitmap.sum())) == (0, 0, 0, 1, 0)
    assert not q.y.any() and not torch.signbit(q.y).any() and not q.channel_bits_q_after.any()
    q = gmc.quantize_rdo(torch.full_like(y, -0.3), s, m, w, 0.5)  # round(y) = -0.0 everywhere: written as +0.0
    assert not q.y.any() and not torch.signbit(q.y).any() and q.bits_q_before == 0
    # an item without latents is a no-op
    e = torch.empty((1, 0, 4, 4), device=DEV)
    q = gmc.quantize_rdo(e, e, e, e, 0.5)
    assert (q.n_changed, q.bits_q_before, q.bits_q_after, q.y.numel()) == (0, 0, 0, 0)


def test_overlapping_output_is_refused():
    """y_rdo is zeroed before the census reads y: any overlap of the two ranges is refused, not only y_rdo == y"""
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    y, s, m, w = (dv(a) for a in T.make_latent(7, 8, 4, 4))
    n = y.numel()
    buf = torch.zeros(3 * n, device=DEV)
    buf[n:2 * n] = y.reshape(-1)
    want = gmc.quantize_rdo(y, s, m, w, 0.5).y.reshape(-1)

    def call(off):  # y in the middle third of buf, y_rdo `off` floats from it
        it = _lib.fgmm_rdoq_item()
        it.y = buf.data_ptr() + 4 * n
        it.y_rdo = it.y + 4 * off
        it.params = _lib.fgmm_params(s.data_ptr(), m.data_ptr(), w.data_ptr(), 8 * 16, 16, _lib.FGMM_F32, 0)
        it.M, it.K, it.hw = 8, 4, 16
        torch.cuda.synchronize()
        return _lib.lib().fgmm_gmc_rdoq_batch(_lib.ctx(0), None, it, 1, 0, 1, 0.5)

    for off in (0, 4, n - 1, -(n - 1)):  # the same range, a shifted one, one float shared at either end
        assert call(off) == 1, off
    torch.cuda.synchronize()
    assert torch.equal(buf[n:2 * n], y.reshape(-1)) and not buf[:n].any() and not buf[2 * n:].any()  # (refused before anything ran)
    for off in (n, -n):  # adjacent ranges do not overlap
        assert call(off) == 0, off
        assert torch.equal(buf[n + off:2 * n + off], want) and torch.equal(buf[n:2 * n], y.reshape(-1))


def test_stacked_tensors_through_the_ctypes_boundary(monkeypatch):
    """without the compiled extension the stacked form builds its items as a numpy record array (RDOQ_ITEM_DTYPE): the same results"""
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    cols = [torch.cat([dv(a) for a in col]) for col in zip(*(T.make_latent(seed, 12, 8, 13, zero_frac=zf) for seed, zf in Q.SEEDS))]
    want = [key(q) for q in gmc.quantize_rdo_batch(*([c[i:i + 1] for i in range(2)] for c in cols), 0.5, per_channel=True)]
    monkeypatch.setattr(_lib, "native", lambda: None)
    for per_channel in (True, False):
        got = gmc.quantize_rdo_batch(*cols, 0.5, per_channel=per_channel)
        assert [key(q)[:None if per_channel else -1] for q in got] == [k[:None if per_channel else -1] for k in want]
        assert all((q.channel_bits_q_after is None) != per_channel for q in got)


# ---- (f) the codecs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantizer", ["noise", "weighted_mean_ste"])
def test_latent_codec_with_rdo_lambda(quantizer):
    """GaussianMixtureConditionalLatentCodec(rdo_lambda) through its own compress: what is coded is quantize_rdo of what the codec
    would round - y itself, or (weighted_mean_ste) y less the mixture's mean - and a codec without the argument decodes it"""
    from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec

    y, s, m, w = T.make_latent(5, 12, 8, 13)
    y, params = dv(y), dv(np.concatenate([s, m, np.log(w)], axis=1))
    codec = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya", rdo_lambda=0.5)
    plain = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya")
    gmc = plain.gaussian_mixture_conditional
    sc, me, we = plain._params(params)
    d, add = y, None
    if quantizer != "noise":
        add, me = plain._recentre(me, we)
        d = y - add
    q = gmc.quantize_rdo(d, sc, me, we, 0.5)
    assert q.n_changed > 0
    enc = codec.compress(y, params)
    (b, am, zb), _ = gmc.compress(q.y, sc, me, we)
    assert torch.equal(enc["y_hat"], q.y)
    assert (bytes(enc["strings"][0][0]), enc["strings"][0][1], enc["strings"][0][2].tolist()) == (bytes(b), am, zb.tolist())
    assert bytes(plain.compress(y, params)["strings"][0][0]) != bytes(b)
    want = q.y if add is None else q.y + add
    for decoder in (codec, plain):  # an encoder-side choice: the decoder needs no switch
        assert torch.equal(decoder.decompress(enc["strings"], enc["shape"], params)["y_hat"], want)


# ---- the checkerboard codec ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_checkerboard_codec_with_rdo_lambda(mode):
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    Ctx, Par = T.exact_modules()
    for seed, c, c_side, h, w, dead, parity in ((11, 6, 8, 8, 12, 0, "even"), (12, 5, 6, 6, 10, 1, "odd")):
        y, side = T.exact_codec_inputs(seed, c, c_side, h, w, dead=dead)

        def make(**kw):
            return CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, quantizer="noise", mode=mode)},
                                           context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c), anchor_parity=parity, **kw).cuda()

        codec = make(rdo_lambda=0.5)
        enc = codec.compress(dv(y), dv(side))
        dec = codec.decompress(enc["strings"], enc["shape"], dv(side))
        assert torch.equal(dec["y_hat"], enc["y_hat"]), seed
        # the same, half by half: each half's latents quantised with the parameters its context gives, the non-anchors' context made
        # of the anchors' RDOQ result
        inner, gmc = codec.latent_codec["y"], codec.latent_codec["y"].gaussian_mixture_conditional
        y_, side_ = codec.unembed(dv(y)), codec.unembed(dv(side))
        y_hat_ = side_.new_zeros((2, 1, c, h, w // 2))
        moved = 0
        for i in range(2):
            params_i = codec.entropy_parameters(codec.merge(codec._ctx(y_hat_, i), side_[i]))
            _, sc, me, we = inner.coder_inputs_rdo(y_[i], params_i, 0.0)
            q = gmc.quantize_rdo(y_[i], sc, me, we, 0.5)
            y_hat_[i] = q.y
            moved += q.n_changed
        assert torch.equal(codec.embed(y_hat_), enc["y_hat"]), seed
        assert moved > 0 and not torch.equal(enc["y_hat"], torch.round(dv(y))), seed
        # rdo_lambda = 0 is today's path: byte-identical to a codec constructed without the argument
        a, b = make(rdo_lambda=0.0).compress(dv(y), dv(side)), make().compress(dv(y), dv(side))
        assert [bytes(s[0]) for s in a["strings"]] == [bytes(s[0]) for s in b["strings"]] and torch.equal(a["y_hat"], b["y_hat"])
        assert [bytes(s[0]) for s in a["strings"]] != [bytes(s[0]) for s in enc["strings"]]
