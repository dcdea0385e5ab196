"""GPU (-m gpu): the HIP paths against the COMPILED reference (oracle/_ref, run by tests/ref_worker.py in a CPU-only child per
mode) on the edge corpus of tests/edge_corpus.py.  The expected answer is always the reference's, never the oracle's: the float
CDF, the bytes of RansEncoder / compress_batch (fp32, fp16 and logit planes), and the symbols of every decoder - RansDecoder,
decompress_batch with both table kernels, the host workers and the GPU segment decoder - on garbage, truncated and corrupted
streams; a decoder fails exactly where the reference reads past the end of the stream.  At the API level the latents go
through compress / decompress, checked against the reference's quantisation lines as torch CPU ops."""
import functools

import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, _lib, ans
from oracle import oracle as O
from tests import edge_corpus as E
from tests import ref_worker as W
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
N_CDF = 4096
M_D, H_D, W_D = 8, 16, 16      # the decode cases: 2048 latents, 7 checkpoints at stride 256
N_D = M_D * H_D * W_D
Y_CLIP = 60                     # |y| of the decode cases' latents: abs_max <= 61
DEC_BS = (5, 37, 127, 200)
API_DECODE_MAX = 40000          # latent families decoded at the API level (abs_max beyond: compressed only)


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _planes(rows, M=M_D, h=H_D, w=W_D):
    """rows [M*h*w, 4] (channel-major latents) -> plane [1, 4M, h, w], component k at channel k*M + c"""
    return np.ascontiguousarray(rows.reshape(M, h, w, 4).transpose(3, 0, 1, 2).reshape(1, 4 * M, h, w))


def _ref_quant(y):
    """the reference's quantisation lines (entropy_models.py:834-846) as torch CPU ops -> (abs_max, zero_bitmap, symbols, y_q)"""
    yt = torch.from_numpy(np.ascontiguousarray(y))
    abs_max = max(torch.abs(yt.max()).int().item(), torch.abs(yt.min()).int().item()) + 1
    abs_max = 1 if abs_max < 1 else abs_max
    yq = torch.round(yt)
    zb = torch.where(torch.sum(torch.abs(yq), (3, 2)).squeeze(0) == 0, 0, 1)
    nonzero = torch.nonzero(zb).flatten().tolist()
    return abs_max, zb, yq[:, nonzero].reshape(-1).int().numpy(), yq.numpy()


def _rows_of(y, s, m, w, clamp):
    """the parameter rows the reference codes with (reshape_entropy_parameters, entropy_models.py:810-828)"""
    _, s2, m2, w2, *_ = T.to_coder_inputs(y, s, m, w, clamp=clamp)
    return [np.ascontiguousarray(a, np.float32) for a in (s2, m2, w2)]


def _softmax_dev(logit_planes):
    """the device's own pi for logits (fgmm_softmax4_hip), as planes"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    M = logit_planes.shape[1] // 4
    h, w = logit_planes.shape[2:]
    rows = dv(logit_planes.reshape(4, -1).T)
    out = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), out.data_ptr(), rows.size(0)))
    return np.ascontiguousarray(out.cpu().numpy().T.reshape(1, 4 * M, h, w))


def gpu_cdf(mode, v, s, m, w):
    L, ctx = _lib.lib(), _lib.ctx(0)
    v, s, m, w = dv(v.astype(np.int32)), dv(s), dv(m), dv(w)
    n = v.numel()
    c1 = torch.empty(n, dtype=torch.float32, device=DEV)
    c2 = torch.empty_like(c1)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_gmm_cdf_hip(ctx, None, v.data_ptr(), s.data_ptr(), m.data_ptr(), w.data_ptr(), n, s.stride(0),
                                  s.stride(1), _lib.mode_id(mode), c1.data_ptr(), c2.data_ptr()))
    return c1.cpu().numpy(), c2.cpu().numpy()


def _decode_inputs(fam):
    """a latent item [1, M_D, H_D, W_D] with the family's parameters: y = the family's symbols, clipped"""
    c = E.param_case(fam)
    y = np.clip(c["v"][:N_D], -Y_CLIP, Y_CLIP).astype(np.float32).reshape(1, M_D, H_D, W_D)
    return y, _planes(c["s"][:N_D]), _planes(c["m"][:N_D]), _planes(c["w"][:N_D])


def _streams(fam, valid):
    """the corpus' streams of a checkpointed bitstream: "flipped" also corrupts its last segment alone (8 + 4 * pos: the words
    the decoder has not read when it stands at the last note) - what only the GPU segment decoder's own checks decide"""
    tail = 8 + 4 * int(valid.ckpt["pos"][-1])
    return ([("valid", bytes(valid))] if fam == "truncated" else []) + E.stream_cases(fam, bytes(valid), N_D, tail_from=tail)


@functools.lru_cache(maxsize=None)
def _prepared(mode, tmp):
    """-> (cases, product-side encodes, reference answers) of one mode; the decode cases' streams are the product's bitstreams
    (whose bytes are themselves checked against the reference's) and what edge_corpus derives from them"""
    cases, prod = {}, {}
    for fam in E.PARAM_FAMILIES:
        c = E.param_case(fam, n=N_CDF)
        cases[f"{fam}.cdf"] = {"kind": "cdf", "v": c["v"], "s": c["s"], "m": c["m"], "w": c["w"]}
        cases[f"{fam}.cdfx"] = {"kind": "cdf_x", "x1": c["x1"], "x2": c["x2"], "s": c["s"], "m": c["m"], "w": c["w"]}
        cases[f"{fam}.enc"] = {"kind": "encode", "v": c["v"], "s": c["s"], "m": c["m"], "w": c["w"]}
        # decode cases: the item coded by the product with checkpoints (clamp off: the family's parameters as they are)
        y, s, m, w = _decode_inputs(fam)
        ck = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=False, checkpoint_stride=256)
        (b, am, zb), _ = ck.compress(*(dv(a) for a in (y, s, m, w)))
        prod[fam] = (b, am, zb.cpu())
        sym = _ref_quant(y)[2]
        rows = _rows_of(y, s, m, w, clamp=False)
        cases[f"{fam}.dec_enc"] = {"kind": "encode", "v": sym, "s": rows[0], "m": rows[1], "w": rows[2]}
        for sf in E.STREAM_FAMILIES:
            for tag, bb in _streams(sf, b):
                for bs in DEC_BS + (am + 1,):
                    cases[f"{fam}.{sf}.{tag}.{bs}"] = {"kind": "decode", "bytes": np.frombuffer(bb, np.uint8), "s": rows[0],
                                                       "m": rows[1], "w": rows[2], "max_bs": np.int32(bs)}
    for fam in E.FP16_FAMILIES:
        y, s16, m16, w16 = E.fp16_case(fam)
        sym = _ref_quant(y)[2]
        rows = _rows_of(y, *(a.astype(np.float32) for a in (s16, m16, w16)), clamp=True)
        cases[f"{fam}.enc"] = {"kind": "encode", "v": sym, "s": rows[0], "m": rows[1], "w": rows[2]}
        # the same planes in fp32 with the weights given as logits: the reference is fed the device's own softmax
        lg = np.log(np.maximum(np.nan_to_num(w16.astype(np.float32), nan=0.0), 1e-30)).astype(np.float32)
        pi_dev = _softmax_dev(lg)
        rows = _rows_of(y, s16.astype(np.float32), m16.astype(np.float32), pi_dev, clamp=True)
        cases[f"{fam}.logits.enc"] = {"kind": "encode", "v": sym, "s": rows[0], "m": rows[1], "w": rows[2]}
        prod[f"{fam}.logits"] = lg
    for fam in E.LATENT_FAMILIES:
        y, s, m, w = E.latent_case(fam)
        am, _, sym, _ = _ref_quant(y)
        rows = _rows_of(y, s, m, w, clamp=True)
        cases[f"lat_{fam}.enc"] = {"kind": "encode", "v": sym, "s": rows[0], "m": rows[1], "w": rows[2]}
        if am + 1 <= API_DECODE_MAX:
            gmc = GaussianMixtureConditional(K=4, mode=mode, checkpoint_stride=256)
            (b, am_p, zb_p), _ = gmc.compress(*(dv(a) for a in (y, s, m, w)))
            prod[f"lat_{fam}"] = (bytes(b), am_p, zb_p.cpu())
            # the reference decodes the product's stream with the product's side information: checked against the
            # reference's own in test_api_level_latents
            zb_np = zb_p.cpu().numpy()
            nz = np.nonzero(zb_np)[0]
            rs = [np.ascontiguousarray(a.reshape(4, -1, a.shape[2] * a.shape[3])[:, nz].reshape(4, -1).T) for a in (s, m, w)]
            rs[0] = np.clip(rs[0], np.float32(0.11), np.float32(256))
            cases[f"lat_{fam}.dec"] = {"kind": "decode", "bytes": np.frombuffer(bytes(b), np.uint8), "s": rs[0], "m": rs[1],
                                       "w": rs[2], "max_bs": np.int32(am_p + 1)}
    for fam in SEG_TAIL_FAMILIES:
        y, s, m, w = _seg_tail_inputs(fam)
        ck = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=False, checkpoint_stride=256)
        (b, am, zb), _ = ck.compress(*(dv(a) for a in (y, s, m, w)))
        prod[f"seg_{fam}"] = (b, am, zb.cpu())
        rows = _rows_of(y, s, m, w, clamp=False)
        cases[f"seg_{fam}.enc"] = {"kind": "encode", "v": _ref_quant(y)[2], "s": rows[0], "m": rows[1], "w": rows[2]}
        for tag, bb in _seg_tail_streams(b):
            cases[f"seg_{fam}.{tag}"] = {"kind": "decode", "bytes": np.frombuffer(bb, np.uint8), "s": rows[0], "m": rows[1],
                                         "w": rows[2], "max_bs": np.int32(am + 1)}
    return cases, prod, W.run(mode, cases, tmp)


# The GPU segment decoder leaves a row that decreases somewhere to the table path (the reference's bisection): in such a row a
# count of the edges <= cf need not be the bisection's interval.  A wrong symbol in any segment but the last is caught by the
# next note, and the whole item goes through the table path anyway; the LAST segment is verified against no note.  So these
# items are ordinary up to the last note (latent 7 * 256) and hold the family's rows - non-monotone ones among them - after it.
# neg_sigma / neg_weights rows mostly also fall into their saturated tail, which the kernel refuses on its own; dip_weights
# rows decrease only inside the window, where nothing but the non-monotone flag sends them back.  A wrong symbol there leaves
# the coder state wrong, and the next such row is then likely to be refused for another reason: so dip_weights is also drawn
# with only the item's last 8 rows its own (n_head 2040), and decoded from many replaced tails.
SEG_TAIL_CASES = (("neg_sigma", 1792), ("neg_weights", 1792), ("nan_weights", 1792), ("dip_weights", 1792), ("dip_weights", 2040))
SEG_TAIL_FAMILIES = tuple(f"{f}-{h}" for f, h in SEG_TAIL_CASES)


def _seg_tail_inputs(case):
    fam, n_head = case.rsplit("-", 1)
    c = E.param_case_after(fam, N_D, int(n_head))
    y = np.clip(c["v"], -Y_CLIP, Y_CLIP).astype(np.float32).reshape(1, M_D, H_D, W_D)
    return y, _planes(c["s"]), _planes(c["m"]), _planes(c["w"])


def _seg_tail_streams(b):
    """the valid stream, and the stream with the words of its last segment only replaced (edge_corpus's "tail" cases)"""
    tail = 8 + 4 * int(b.ckpt["pos"][-1])
    tails = [(f"s{k}{t}", bb) for k in range(8) for t, bb in E.stream_cases("flipped", bytes(b), N_D, seed=k, tail_from=tail)
             if t.startswith("tail")]
    return [("valid", bytes(b))] + tails


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    assert O.ref_available(), "oracle/_ref is missing: build() makes it and the files travel with the tree"

    def get(mode):
        return _prepared(mode, str(tmp_path_factory.getbasetemp()))

    return get


def _differ(got, want):
    """bit for bit, except that a NaN equals any NaN: x86 makes the negative default NaN where the GPU makes the positive one,
    and no NaN's bits reach a stream (both quantise it to the same edge)"""
    g, w = (np.ascontiguousarray(a, np.float32) for a in (got, want))
    return (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))


@pytest.mark.parametrize("fam", list(E.PARAM_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_float_cdf_equals_compiled_reference(prep, mode, fam):
    cases, _, ref = prep(mode)
    x = cases[f"{fam}.cdf"]
    c1, c2 = gpu_cdf(mode, x["v"], x["s"], x["m"], x["w"])
    want = ref[f"{fam}.cdf"]
    bad = np.nonzero(_differ(c1, want["c1"]) | _differ(c2, want["c2"]))[0]
    assert len(bad) == 0, (len(bad), bad[:5], c1[bad[:3]], want["c1"][bad[:3]])


@pytest.mark.parametrize("fam", list(E.PARAM_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_encoders_equal_compiled_reference(prep, mode, fam):
    """RansEncoder on GPU tensors (symbols anywhere in int32), and compress of the decode item, against the reference's bytes"""
    cases, prod, ref = prep(mode)
    x = cases[f"{fam}.enc"]
    got = ans.RansEncoder().encode_with_indexes_gmm(dv(x["v"]), dv(x["s"]), dv(x["m"]), dv(x["w"]), 0, mode=mode)
    assert got == ref[f"{fam}.enc"]["bytes"].tobytes()
    assert bytes(prod[fam][0]) == ref[f"{fam}.dec_enc"]["bytes"].tobytes()


@pytest.mark.parametrize("fam", list(E.FP16_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_compress_batch_fp16_and_logit_planes(prep, mode, fam):
    """compress_batch with fp16 planes (the reference fed the widened values), fp32 planes and the weights as logits (the
    reference fed the device's own softmax): the reference's bytes, abs_max and zero_bitmap"""
    _, prod, ref = prep(mode)
    y, s16, m16, w16 = E.fp16_case(fam)
    am, zb, _, yq = _ref_quant(y)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    ((b, am_g, zb_g), yq_g), = gmc.compress_batch([dv(y)], [dv(s16)], [dv(m16)], [dv(w16)])
    assert b == ref[f"{fam}.enc"]["bytes"].tobytes()
    assert am_g == am and zb_g.cpu().tolist() == zb.tolist() and np.array_equal(yq_g.cpu().numpy(), yq)
    f32 = [dv(a.astype(np.float32)) for a in (s16, m16)]
    ((b32, _, _), _), = gmc.compress_batch([dv(y)], [f32[0]], [f32[1]], [dv(w16.astype(np.float32))])
    assert b32 == b
    ((bl, am_l, _), _), = gmc.compress_batch([dv(y)], [f32[0]], [f32[1]], [dv(prod[f"{fam}.logits"])], weights_are_logits=True)
    assert bl == ref[f"{fam}.logits.enc"]["bytes"].tobytes() and am_l == am


def _outcome(fn):
    try:
        return fn()
    except RuntimeError:
        return None


def _check(got, want, what, as_float=False):
    """a decoder fails exactly where the reference depends on words past the end of the stream, else gives its symbols
    (as_float: y_hat, the symbols as float32 - the reference's decompress makes the same conversion)"""
    if int(want["past_end"]):
        assert got is None, f"{what}: decoded where the reference reads past the end of the stream"
    else:
        assert got is not None, f"{what}: failed where the reference decodes within the stream"
        syms = want["syms"].astype(np.float32) if as_float else want["syms"]
        assert np.array_equal(got, syms), (what, np.nonzero(got != syms)[0][:5])


@pytest.mark.parametrize("sf", E.STREAM_FAMILIES)
@pytest.mark.parametrize("fam", list(E.PARAM_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_decoders_equal_compiled_reference(prep, ctx_options, mode, fam, sf):
    """every decoder on garbage / truncated / flipped streams: RansDecoder at several max_bs; at the item's own abs_max,
    decompress_batch (single-pass table kernel, and the generic one), the host workers and the GPU segment decoder"""
    cases, prod, ref = prep(mode)
    b0, am, zb = prod[fam]
    y, s, m, w = _decode_inputs(fam)
    t = [dv(a) for a in (s, m, w)]
    rows = [dv(cases[f"{fam}.dec_enc"][k]) for k in ("s", "m", "w")]
    plain = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=False)
    ck = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=False, checkpoint_stride=256)
    nz = np.nonzero(zb.numpy())[0]
    cap0 = _lib.get_option(0, "tab_cap_e")
    for tag, bb in _streams(sf, b0):
        for bs in DEC_BS + (am + 1,):
            name = f"{fam}.{sf}.{tag}.{bs}"
            want = ref[name]
            got = _outcome(lambda: ans.RansDecoder().decode_with_indexes_gmm(bb, *rows, bs, mode=mode).numpy())
            _check(got, want, name + " RansDecoder")
        want = ref[f"{fam}.{sf}.{tag}.{am + 1}"]

        def as_syms(y_hat):
            return None if y_hat is None else y_hat.cpu().numpy()[0, nz].reshape(-1)

        for what, opts, codec, stream in (("tab", {}, plain, bb), ("generic", {"tab_cap_e": 256}, plain, bb),
                                          ("host workers", {"gpu_decode": 2}, ck, CheckpointedBytes(bb, b0.ckpt, 256)),
                                          ("segment decoder", {"gpu_decode": 1}, ck, CheckpointedBytes(bb, b0.ckpt, 256))):
            ctx_options(**{"tab_cap_e": cap0, "gpu_decode": 0, **opts})
            y_hat = _outcome(lambda: codec.decompress_batch([stream], [am], [zb], [t[0]], [t[1]], [t[2]])[0])
            _check(as_syms(y_hat), want, f"{fam}.{sf}.{tag} {what}", as_float=True)
        ctx_options(gpu_decode=0)


@pytest.mark.parametrize("fam", list(E.LATENT_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_api_level_latents(prep, ctx_options, mode, fam):
    """GaussianMixtureConditional.compress / decompress of the latent families: abs_max, zero_bitmap, y_q (NaN where the
    reference has NaN) and the bytes are the reference's; the decoder, given that abs_max, returns the reference decoder's
    symbols - through the table path, and through the GPU segment decoder where the item's width lets it take the stream"""
    _, prod, ref = prep(mode)
    y, s, m, w = E.latent_case(fam)
    am, zb, sym, yq = _ref_quant(y)
    gmc = GaussianMixtureConditional(K=4, mode=mode, checkpoint_stride=256)
    t = [dv(a) for a in (y, s, m, w)]
    (b, am_g, zb_g), yq_g = gmc.compress(*t)
    assert am_g == am, (am_g, am)
    assert zb_g.cpu().tolist() == zb.tolist()
    assert np.array_equal(yq_g.cpu().numpy(), yq, equal_nan=True)
    assert b == ref[f"lat_{fam}.enc"]["bytes"].tobytes()
    if fam == "one_nan":
        assert am_g == 1  # y.max() is NaN in torch: .int() -> INT32_MIN, floored at 1
    if am + 1 > API_DECODE_MAX:
        return
    want = ref[f"lat_{fam}.dec"]
    assert int(want["past_end"]) == 0
    nz = np.nonzero(zb.numpy())[0]
    seg_ok = len(b.ckpt) > 0 and 2 * (am_g + 1) + 2 <= 2048  # what the segment decoder takes (fgmm_decode_gpu.cpp)
    if fam.startswith("segdec_am"):
        assert len(b.ckpt) > 0 and seg_ok == (fam == "segdec_am_1022")
    for how in (2, 1):  # the host workers' table path, the GPU segment decoder
        ctx_options(gpu_decode=how)
        y_hat = gmc.decompress(b, am_g, zb_g, *t[1:]).cpu().numpy()
        assert np.array_equal(y_hat[0, nz].reshape(-1), want["syms"].astype(np.float32)), how
        assert not np.any(y_hat[0, np.nonzero(zb.numpy() == 0)[0]])
        if how == 1:  # given to the segment decoder (decoded there, or handed back) exactly when its width allows
            assert _lib.ctx_stat(0, 4) + _lib.ctx_stat(0, 5) == int(seg_ok), (_lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5))


@pytest.mark.parametrize("fam", SEG_TAIL_FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_segment_decoder_last_segment_equals_compiled_reference(prep, ctx_options, mode, fam):
    """items ordinary up to their last note with the family's (partly non-monotone) rows after it, decoded from the valid stream
    and from streams whose last segment alone is replaced: the GPU segment decoder (which must hand such rows back) and the
    table path give the reference's symbols"""
    cases, prod, ref = prep(mode)
    b, am, zb = prod[f"seg_{fam}"]
    assert bytes(b) == ref[f"seg_{fam}.enc"]["bytes"].tobytes()
    assert zb.tolist() == [1] * M_D and len(b.ckpt) == 7 and 2 * (am + 1) + 2 <= 2048
    _, s, m, w = _seg_tail_inputs(fam)
    t = [dv(a) for a in (s, m, w)]
    ck = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=False, checkpoint_stride=256)
    for tag, bb in _seg_tail_streams(b):
        want = ref[f"seg_{fam}.{tag}"]
        for how in (1, 2):
            ctx_options(gpu_decode=how)
            y_hat = _outcome(lambda: ck.decompress_batch([CheckpointedBytes(bb, b.ckpt, 256)], [am], [zb], *([a] for a in t))[0])
            _check(None if y_hat is None else y_hat.cpu().numpy().reshape(-1), want, f"seg_{fam}.{tag} gpu_decode={how}",
                   as_float=True)
            if how == 1 and y_hat is not None:
                assert _lib.ctx_stat(0, 4) + _lib.ctx_stat(0, 5) == 1  # the item went to the segment decoder


@pytest.fixture
def ctx_options():
    """set options of the process-wide context for one test and restore them afterwards"""
    saved = {}

    def set_(**kw):
        for k, v in kw.items():
            saved.setdefault(k, _lib.get_option(0, k))
            _lib.set_option(0, k, v)

    yield set_
    for k, v in saved.items():
        _lib.set_option(0, k, v)
