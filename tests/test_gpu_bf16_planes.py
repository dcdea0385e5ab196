"""GPU (-m gpu): bfloat16 parameter planes (include/flashgmm_amd.h section 2, FGMM_BF16) in every call that takes planes.

Every assertion compares two runs: the call on bfloat16 planes P16, and the same call on P16.float() - the float32 instantiations, which
this form leaves untouched, fed the widened values.  The contract is exact equality of every output.  compress is, besides, compared with
the CPU oracle on the widened values.  The inputs are tests/bf16_planes.py's (their precondition, sum of the widened weights <= 1, is
checked by tests/test_bf16_planes_cpu.py); each shape is a call of its own so that it reaches the kernel form its name says."""
import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from tests import bf16_planes as B
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
LAMBDAS16 = [0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 16.0]
ITEMS = B.items()


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bf(bits, offset=False):
    """bfloat16 bit patterns -> a device tensor of that dtype; offset: a dense view that starts two bytes into its storage"""
    t = torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)
    if offset:
        buf = torch.zeros(t.numel() + 1, dtype=torch.bfloat16, device=DEV)
        buf[1:] = t.reshape(-1)
        t = buf[1:].view(t.shape)
        assert t.data_ptr() % 16 == 2
    return t


def wide_of(p16, offset=False):
    """P16.float(), the planes of the float32 run: bit for bit the widened values; offset: as misaligned as the bfloat16 planes are"""
    out = []
    for t in p16:
        f = t.float()
        assert torch.equal(f.view(torch.int32), t.view(torch.int16).to(torch.int32) << 16)
        if offset:
            buf = torch.zeros(f.numel() + 1, dtype=torch.float32, device=DEV)
            buf[1:] = f.reshape(-1)
            f = buf[1:].view(f.shape)
        out.append(f)
    return out


def inputs(name, logits):
    """-> y (device), P16, P32, and the host's widened (sigma, mu, weights-or-logits)"""
    y, sg, mu, pi = ITEMS[name]
    bits = B.planes_bits(sg, mu, pi, logits)
    off = name in B.OFFSET_VIEW
    p16 = [bf(b, off) for b in bits]
    return dv(y), p16, wide_of(p16, off), [B.widen(b) for b in bits]


def softmax_dev(logit_planes):
    """the device's own pi for logits (fgmm_softmax4_hip: the kernels' fixed binary32 sequence), as planes"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    M = logit_planes.shape[1] // 4
    h, w = logit_planes.shape[2:]
    rows = dv(logit_planes.reshape(4, -1).T)
    out = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), out.data_ptr(), rows.size(0)))
    return np.ascontiguousarray(out.cpu().numpy().T.reshape(1, 4 * M, h, w))


def same(a, b):
    """equality of two results, field by field; floats bit for bit (a NaN equals itself)"""
    if isinstance(a, torch.Tensor):
        if not (isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape):
            return False
        if a.dtype == torch.float32:
            return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
        return torch.equal(a, b)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    slots = [s for c in type(a).__mro__ for s in getattr(c, "__slots__", ())]
    if slots and not isinstance(a, (bytes, str)):
        return type(a) is type(b) and all(same(getattr(a, s), getattr(b, s)) for s in slots)
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    return type(a) is type(b) and a == b


def enc_key(res):
    (b, am, zb), yq = res
    ck = getattr(b, "ckpt", None)
    return (bytes(b), int(am), zb.cpu().tolist(), yq.cpu().numpy().tobytes(), None if ck is None else ck.tobytes())


def outcome(f):
    """what a call does: its value, or the message of the error it raises"""
    try:
        return ("ok", f())
    except RuntimeError as e:
        return ("raised", str(e))


@pytest.fixture
def ctx_options():
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


# ---- compress and decompress -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_compress_and_decompress_equal_the_float32_run_and_the_oracle(oracle, mode, clamp, logits):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for name in B.SHAPES:
        y, p16, p32, host = inputs(name, logits)
        assert p16[0].dtype == torch.bfloat16 and p32[0].dtype == torch.float32
        got = gmc.compress(y, *p16, weights_are_logits=logits)
        want = gmc.compress(y, *p32, weights_are_logits=logits)
        assert enc_key(got) == enc_key(want), name
        (b, am, zb), yq = got
        assert zb[B.DEAD] == 0 and zb[B.OUTLIER] == 1, name
        assert gmc.estimate_bits(y, *p16, weights_are_logits=logits).n_bypass > 0, name  # the outlier takes the escape
        pi = softmax_dev(host[2]) if logits else host[2]
        sym, s, m, wt, am_, zb_, yq_ = T.to_coder_inputs(ITEMS[name][0], host[0], host[1], pi, clamp=clamp)
        assert bytes(b) == oracle.encode_gmm(mode, sym, s, m, wt), name
        assert (am, zb.cpu().tolist()) == (am_, zb_.tolist()) and np.array_equal(yq.cpu().numpy(), yq_), name
        d16 = gmc.decompress(b, am, zb, *p16, weights_are_logits=logits)
        d32 = gmc.decompress(b, am, zb, *p32, weights_are_logits=logits)
        assert same(d16, d32) and torch.equal(d16, yq), name


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_special_values_equal_the_float32_run(mode, clamp, logits):
    """sigma at 1e-5 and 3e3, a subnormal mean, -0.0 and a NaN sigma: whatever the float32 path makes of the widened values - the bytes,
    and a decode that returns or fails - the bfloat16 path makes of them too"""
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    y, p16, p32, host = inputs("special", logits)
    assert np.isnan(host[0]).sum() == 1 and (host[0][np.isfinite(host[0])] > 2e3).any() and (host[0] < 2e-5).any()
    assert ((host[1] != 0) & (np.abs(host[1]) < 1e-38)).any() and (host[1].view(np.uint32) == 0x80000000).any()
    got = gmc.compress(y, *p16, weights_are_logits=logits)
    want = gmc.compress(y, *p32, weights_are_logits=logits)
    assert enc_key(got) == enc_key(want)
    (b, am, zb), yq = got
    d16 = outcome(lambda: gmc.decompress(b, am, zb, *p16, weights_are_logits=logits))
    d32 = outcome(lambda: gmc.decompress(b, am, zb, *p32, weights_are_logits=logits))
    assert d16[0] == d32[0] and same(d16[1], d32[1])
    for f in (lambda p: gmc.estimate_bits(y, *p, weights_are_logits=logits, per_channel=True, per_latent=True),
              lambda p: gmc.quantize_rdo(y, *p, 0.5, weights_are_logits=logits, per_channel=True),
              lambda p: gmc.rd_curve(y, *p, LAMBDAS16, weights_are_logits=logits)):
        assert same(f(p16), f(p32))


@pytest.mark.parametrize("binding", ["compiled", "ctypes"])
def test_batches_stacked_and_as_sequences_in_both_bindings(monkeypatch, binding):
    """the stacked form (one pointer and a stride per plane: the element size enters) and the sequence form, through the compiled
    boundary and through ctypes: one result"""
    if binding == "ctypes":
        monkeypatch.setattr(_lib, "_native", False)
        assert _lib.native() is None
    else:
        assert _lib.native() is not None
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    names = ["stack0", "stack1", "stack2"]
    ys = torch.cat([dv(ITEMS[n][0]) for n in names])
    bits = [B.planes_bits(*ITEMS[n][1:], False) for n in names]
    s16 = [torch.cat([bf(b[j]) for b in bits]) for j in range(3)]  # [N, K*M, h, w]
    s32 = wide_of(s16)
    assert ys.shape[0] == 3 and s16[0].shape[0] == 3
    runs = {}
    for what, p in (("bf16", s16), ("f32", s32)):
        stacked = gmc.compress_batch(ys, *p)
        seq = gmc.compress_batch([y[None] for y in ys], *[[t[i:i + 1] for i in range(3)] for t in p])
        runs[what] = ([enc_key(r) for r in stacked], [enc_key(r) for r in seq])
        strings, ams, zbs = [r[0][0] for r in stacked], [r[0][1] for r in stacked], [r[0][2] for r in stacked]
        out_st = gmc.decompress_batch(strings, ams, torch.stack(zbs), *p)
        out_sq = gmc.decompress_batch(strings, ams, zbs, *[[t[i:i + 1] for i in range(3)] for t in p])
        for i in range(3):
            assert torch.equal(out_st[i].reshape(ys[i].shape), torch.round(ys[i])) and torch.equal(out_sq[i].reshape(ys[i].shape), torch.round(ys[i])), (what, i)
        est = gmc.estimate_bits_batch(ys, *p, per_channel=True)
        rdo = gmc.quantize_rdo_batch(ys, *p, 0.5)
        runs[what] += (est, rdo)
    a, b = runs["bf16"], runs["f32"]
    assert a[0] == a[1] == b[0] == b[1]
    assert same(a[2], b[2]) and same(a[3], b[3])
    # each item alone is the same stream: the batch's strides and pointers name the right planes
    for i, n in enumerate(names):
        assert enc_key(gmc.compress(ys[i:i + 1], *[t[i:i + 1] for t in s16])) == a[0][i], n


def test_a_batch_of_mixed_plane_types_is_refused(monkeypatch):
    """either binding hands each item's dtype to the library as it is, and the library refuses the mix"""
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    y, p16, p32, _ = inputs("v8_tiled", False)
    h16 = [t.half() for t in p32]
    (b, am, zb), _ = gmc.compress(y, *p16)
    for error in (RuntimeError, _lib.FgmmError):  # the compiled binding, then ctypes
        if error is _lib.FgmmError:
            monkeypatch.setattr(_lib, "_native", False)
        assert (_lib.native() is None) == (error is _lib.FgmmError)
        for other in (h16, p32):
            cols = [[a, o] for a, o in zip(p16, other)]
            for call in (lambda: gmc.compress_batch([y, y], *cols), lambda: gmc.estimate_bits_batch([y, y], *cols),
                         lambda: gmc.quantize_rdo_batch([y, y], *cols, 0.5), lambda: gmc.rd_curve_batch([y, y], *cols, [0.5]),
                         lambda: gmc.quantize_to_budget_batch([y, y], *cols, 100), lambda: gmc.decompress_batch([b, b], [am, am], [zb, zb], *cols)):
                with pytest.raises(error, match="FGMM_ERR_INVALID"):
                    call()


# ---- the decode side --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_generic_table_form_above_half_width_511(mode, clamp):
    """abs_max = 601: the item does not fit tab_kernel and takes cdftab_count_kernel / cdftab_fill_kernel"""
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    y, p16, p32, _ = inputs("wide", False)
    got, want = gmc.compress(y, *p16), gmc.compress(y, *p32)
    assert enc_key(got) == enc_key(want)
    (b, am, zb), yq = got
    assert am == 601
    d16, d32 = gmc.decompress(b, am, zb, *p16), gmc.decompress(b, am, zb, *p32)
    assert same(d16, d32) and torch.equal(d16, yq)


@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_segment_decoder_settles_the_item_itself(ctx_options, mode, clamp):
    """segdec_kernel on bfloat16 planes: checkpointed every 256 symbols, decoded on the GPU - and (1, 0): by the kernel itself, not by the
    table path that would take over (and hide) a segment that fails its note"""
    ctx_options(gpu_decode=1)
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp, checkpoint_stride=256)
    y, p16, p32, _ = inputs("segdec", False)
    got, want = gmc.compress(y, *p16), gmc.compress(y, *p32)
    assert enc_key(got) == enc_key(want)
    (b, am, zb), yq = got
    assert len(b.ckpt) == (int(zb.sum()) * y.shape[2] * y.shape[3] - 1) // 256 > 8
    d16 = gmc.decompress(b, am, zb, *p16)
    assert (_lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5)) == (1, 0)
    d32 = gmc.decompress(b, am, zb, *p32)
    assert (_lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5)) == (1, 0)
    assert same(d16, d32) and torch.equal(d16, yq)


# ---- the calls that price latents -----------------------------------------------------------------------------------------------------
def forms(y):
    """keyword arguments of the plain, the weighted and the skip forms for a one-item sequence of y's shape"""
    M, h, w = y.shape[1:]
    cw = dv(np.linspace(0.5, 2.0, M).astype(np.float32))
    pw = dv((0.25 + (np.arange(h * w) % 7) / 4.0).astype(np.float32).reshape(h, w))
    return {"plain": {}, "weighted": dict(channel_weights=cw, position_weights=[pw]), "skip": dict(channel_skip=True),
            "weighted+skip": dict(channel_weights=cw, position_weights=[pw], channel_skip=True)}


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_estimate_bits(mode, clamp, logits):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for name in B.SHAPES:
        y, p16, p32, _ = inputs(name, logits)
        kw = dict(weights_are_logits=logits, per_channel=True, per_latent=True)
        got, want = gmc.estimate_bits_batch([y], *[[t] for t in p16], **kw), gmc.estimate_bits_batch([y], *[[t] for t in p32], **kw)
        assert same(got, want) and got[0].bits_q > 0 and got[0].latent_bits is not None and got[0].channel_bits_q is not None, name


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_quantize_rdo(mode, clamp, logits):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    moved = 0
    for name in B.SHAPES:
        y, p16, p32, _ = inputs(name, logits)
        for form, kw in forms(y).items():
            for lam in (0.0, 0.3, 4.0):
                args = dict(weights_are_logits=logits, per_channel=True, **kw)
                got = gmc.quantize_rdo_batch([y], *[[t] for t in p16], lam, **args)
                want = gmc.quantize_rdo_batch([y], *[[t] for t in p32], lam, **args)
                assert same(got, want), (name, form, lam)
                moved += got[0].n_changed
    assert moved > 0


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_rd_curve(mode, clamp, logits):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    for name in B.SHAPES:
        y, p16, p32, _ = inputs(name, logits)
        for form, kw in forms(y).items():
            got = gmc.rd_curve_batch([y], *[[t] for t in p16], LAMBDAS16, weights_are_logits=logits, **kw)
            want = gmc.rd_curve_batch([y], *[[t] for t in p32], LAMBDAS16, weights_are_logits=logits, **kw)
            assert same(got, want) and len(got[0].bits_q_after) == 16 and got[0].n_changed[-1] > 0, (name, form)


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_quantize_to_budget(mode, clamp, logits):
    gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
    searched = 0
    for name in B.SHAPES:
        y, p16, p32, _ = inputs(name, logits)
        budget = int(0.8 * gmc.estimate_bits(y, *p32, weights_are_logits=logits).nbytes)
        for form, kw in forms(y).items():
            args = dict(weights_are_logits=logits, per_channel=True, **kw)
            got = gmc.quantize_to_budget_batch([y], *[[t] for t in p16], budget, **args)
            want = gmc.quantize_to_budget_batch([y], *[[t] for t in p32], budget, **args)
            assert same(got, want), (name, form)
            searched += got[0].lam > 0
    assert searched > 0


# ---- the latent codecs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quantizer", ["noise", "weighted_mean_ste"])
def test_latent_codec_with_bfloat16_planes(quantizer):
    from flashgmm_amd.latent_codecs import GaussianMixtureConditionalLatentCodec

    y, s, m, w = T.make_latent(5, 12, 8, 13)
    y, params = dv(y), dv(np.concatenate([s, m, np.log(w)], axis=1))
    codec = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya", param_dtype=torch.bfloat16)
    gmc = codec.gaussian_mixture_conditional
    enc = codec.compress(y, params)
    dec = codec.decompress(enc["strings"], enc["shape"], params)
    # its strings are the entropy model's on _planes' output: bfloat16 tensors, the weights rounded toward zero
    sc, me, we = codec._params(params)
    d, add = y, None
    if quantizer != "noise":
        add, me = codec._recentre(me, we)
        d = y - add
        d = (torch.round(d) - d) + d  # (quantize_ste, as the codec hands it on)
    assert torch.equal(dec["y_hat"], enc["y_hat"] if add is None else enc["y_hat"] + add)
    planes = codec._planes(sc, me, we)
    assert all(t.dtype == torch.bfloat16 for t in planes)
    assert (planes[2].float() <= we).all() and (planes[2].float().view(1, 4, -1).sum(1) <= 1).all()
    (b, am, zb), yq = gmc.compress(d, *planes)
    assert torch.equal(yq, enc["y_hat"])
    assert (bytes(enc["strings"][0][0]), enc["strings"][0][1], enc["strings"][0][2].tolist()) == (bytes(b), am, zb.tolist())
    # ... and not those of float32 planes: the type is in use
    f32 = GaussianMixtureConditionalLatentCodec(K=4, quantizer=quantizer, mode="polya")
    assert bytes(f32.compress(y, params)["strings"][0][0]) != bytes(b)


@pytest.mark.parametrize("mode", MODES)
def test_checkerboard_codec_over_bfloat16_planes(mode):
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    Ctx, Par = T.exact_modules()
    for seed, c, c_side, h, w, dead, parity in ((11, 6, 8, 8, 12, 0, "even"), (12, 5, 6, 6, 10, 1, "odd")):
        y, side = T.exact_codec_inputs(seed, c, c_side, h, w, dead=dead)
        inner = GaussianMixtureConditionalLatentCodec(K=4, quantizer="noise", mode=mode, param_dtype=torch.bfloat16)
        codec = CheckerboardLatentCodec(latent_codec={"y": inner}, context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c),
                                        anchor_parity=parity).cuda()
        enc = codec.compress(dv(y), dv(side))
        dec = codec.decompress(enc["strings"], enc["shape"], dv(side))
        assert torch.equal(dec["y_hat"], enc["y_hat"]) and torch.equal(enc["y_hat"], torch.round(dv(y))), seed
