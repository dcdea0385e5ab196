"""GPU (-m gpu): the clamped-sigma fast paths (clamp_scales=True: what every real caller runs) against the COMPILED reference
(oracle/_ref through tests/ref_worker.py, one CPU-only child per mode) on the guard families of tests/edge_corpus.py
(CLAMP_FAMILIES), on PARAM_FAMILIES and on the fp16 families.  With the clamp on the kernels run packed-fp32 sequences behind
guards (Sigma4::set's `tame`, mix4_clamped2's 2^11 compare, Phi2<MODE_LOGISTIC>'s reciprocal guard, tab_window's pruning) and
hand back to the IEEE sequence outside them; a wrong guard gives a stream this library decodes and the reference does not.

  encode   compress_batch's bytes, abs_max and zero bitmap in every launch form of symtab_kernel
  tables   fgmm_build_cdftab_hip / fgmm_build_tab_hip with FGMM_TAB_CLAMP, with and without pruning, entry for entry against
           the table of the reference's _fast_gmm_cdf<4> at every edge
  decode   RansDecoder, decompress_batch (single-pass and generic table kernels), the host workers and the GPU segment decoder
           on the product's own stream and on garbage, truncated and corrupted ones

The 8-byte header form (max_bs > 16382) is not reachable through the two table entry points (fgmm_build_cdftab_hip writes
4-byte headers only, fgmm_build_tab_hip's LDS budget ends far below): it is decoded here, from an item with one symbol at 16390."""
import functools

import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, _lib, ans
from oracle import oracle as O
from tests import edge_corpus as E
from tests import ref_worker as W
from tests import synth as T
from tests.test_gpu_parity import gpu_full_table
from tests.test_gpu_reference_edges import (API_DECODE_MAX, MODES, _check, _differ, _outcome, _ref_quant, _rows_of, _softmax_dev,  # noqa: F401
                                            ctx_options, dv)

pytestmark = pytest.mark.gpu

N = 2304                      # rows of an item: 9 * 256 - eight notes at stride 256, the last segment rows 2048 ..
STRIDE = 256
LAYOUTS = {                   # (M, h, w) of the same N rows in channel-major order, and the symtab_kernel form fp32 / fp16 planes take
    "lin": (9, 16, 16),       # hw = 256: linear grid, VEC 4 / VEC 8
    "pc4": (36, 8, 8),        # hw = 64: per-channel grid, VEC 4 / VEC 8 (hw % 8 == 0)
    "h12": (192, 3, 4),       # hw = 12: per-channel grid, VEC 4 / fp16 VEC 4 (hw % 8 == 4)
    "odd": (256, 3, 3),       # hw = 9: VEC 1
}
F32_LAYOUTS = tuple(LAYOUTS)
F16_LAYOUTS = ("lin", "pc4", "h12", "l512")
LAYOUTS["l512"] = (4, 16, 32)  # fp16 items only, the first 2048 rows: hw = 512 = 64 * 8, the linear grid at VEC 8
Y_CLIP = 60                   # PARAM_FAMILIES' symbols lie anywhere in int32: their items code them clipped, as the sibling file does
FAMILIES = list(E.CLAMP_FAMILIES) + list(E.PARAM_FAMILIES)
F16_ITEMS = list(E.FP16_FAMILIES) + [f"{f}.f16" for f in E.CLAMP_FP16_FAMILIES]
WIDE = "guard_2048@16390"     # one symbol at 16390: max_bs 16392, 8-byte headers, the generic kernels
N_TAB, TAB_BS = 32, (61, 200)            # tables: rows per family, max_bs (2-byte and 4-byte headers)
N_TAB_WIDE, TAB_BS_WIDE = 6, (511, 3001, 7000)  # CLAMP_FAMILIES also at the single-pass kernel's last half-width (1024 edges, 16
                                                # latents per block: the spread_means rows mix fast and slow pairs there), and at
                                                # spread_means' own and a wider one, both beyond the LDS budget: generic kernels only
TAB_CASES = [(k, bs) for bs in TAB_BS + TAB_BS_WIDE[:1] for k in ("generic", "tab")] + [("generic", bs) for bs in TAB_BS_WIDE[1:]]
TAB_PARAMS = [(fam, k, bs) for fam in FAMILIES for k, bs in TAB_CASES if bs in TAB_BS or fam in E.CLAMP_FAMILIES]
FGMM_TAB_NO_PRUNE, FGMM_TAB_CLAMP = 1, 2


def _planes(rows, lay):
    M, h, w = LAYOUTS[lay]
    return np.ascontiguousarray(rows.reshape(M, h, w, 4).transpose(3, 0, 1, 2).reshape(1, 4 * M, h, w))


def _rows(fam):
    """-> (v int32 [N], s, m, w [N, 4] float32, sigma pre-clamp)"""
    if fam == WIDE:
        c = E.clamp_case("guard_2048", N)
        c["v"][5] = 16390
    elif fam.endswith(".f16"):
        c = E.clamp_case(fam[:-4], N)
        with np.errstate(over="ignore"):  # (guard_2048's farthest means are infinite as float16)
            c = {"v": c["v"], **{k: c[k].astype(np.float16).astype(np.float32) for k in ("s", "m", "w")}}
    elif fam in E.CLAMP_FAMILIES:
        c = E.clamp_case(fam, N)
    else:
        c = E.param_case(fam, N)
        c["v"] = np.clip(c["v"], -Y_CLIP, Y_CLIP).astype(np.int32)
    return c["v"], c["s"], c["m"], c["w"]


def _item(fam, lay="lin"):
    """-> (y [1, M, h, w] float32, sigma, mu, pi planes [1, 4M, h, w]; float16 planes for the fp16 items)"""
    M, h, w = LAYOUTS[lay]
    if fam in E.FP16_FAMILIES:
        return E.fp16_case(fam, M, h, w)
    v, s, m, p = _rows(fam)
    dt = np.float16 if fam.endswith(".f16") else np.float32
    n = M * h * w
    return (v[:n].astype(np.float32).reshape(1, M, h, w),) + tuple(_planes(a[:n], lay).astype(dt) for a in (s, m, p))


def _f32(a):
    return a.astype(np.float32)


def _logits(w):
    return np.log(np.maximum(np.nan_to_num(_f32(w), nan=0.0), 1e-30)).astype(np.float32)


def _enc_case(y, s, m, w):
    rows = _rows_of(y, _f32(s), _f32(m), _f32(w), clamp=True)
    return {"kind": "encode", "v": _ref_quant(y)[2], "s": rows[0], "m": rows[1], "w": rows[2]}


def _streams(sf, valid, n):
    tail = 8 + 4 * int(valid.ckpt["pos"][-1])
    return ([("valid", bytes(valid))] if sf == "truncated" else []) + E.stream_cases(sf, bytes(valid), n, tail_from=tail)


@functools.lru_cache(maxsize=None)
def _decode_items():
    """name -> (y, planes, weights_are_logits): fp32 planes of every family, fp16 planes, logits planes, the wide item"""
    items = {fam: _item(fam) + (False,) for fam in FAMILIES + [WIDE] + F16_ITEMS}
    for fam in F16_ITEMS:
        y, s, m, w = _item(fam)
        items[f"{fam}.logits"] = (y, _f32(s), _f32(m), _logits(w), True)
    return items


# Families whose weights are a distribution (non-negative, finite, sum <= 1): every row is monotone (a sum of monotone terms, each
# operation rounding monotonically), so on the valid stream every note matches and the segment decoder has no reason to hand the
# bitstream back.  If it does, its producer evaluated an edge differently from the encoder and its own note check caught it - the
# answer is still right (the table path's), only this counter tells.
SEG_SETTLES = ("guard_2048", "spread_means_1022", "spread_means_510", "nan_sigma_one", "sigma_at_clamp", "logistic_rcp_guard", "sat_edges")
DECODE_ITEMS = FAMILIES + [WIDE] + F16_ITEMS + [f"{f}.logits" for f in F16_ITEMS]
# items ordinary up to the last note with the family's rows - rows that decrease under the clamp among them - after it
# (tests/test_gpu_reference_edges.py: SEG_TAIL_CASES)
SEG_TAIL = tuple(E.CLAMP_NONMONO_FAMILIES)
N_HEAD = 8 * STRIDE


def _seg_tail_item(fam):
    c = E.clamp_case_after(fam, N, N_HEAD)
    return (c["v"].astype(np.float32).reshape(1, *LAYOUTS["lin"]),) + tuple(_planes(c[k], "lin") for k in ("s", "m", "w"))


def _seg_tail_streams(b):
    tail = 8 + 4 * int(b.ckpt["pos"][-1])
    return [("valid", bytes(b))] + [(f"s{k}{t}", bb) for k in range(4) for t, bb in E.stream_cases("flipped", bytes(b), N, seed=k, tail_from=tail)
                                    if t.startswith("tail")]


@functools.lru_cache(maxsize=None)
def _prepared(mode, tmp):
    """-> (cases, product-side streams, the reference's answers) of one mode"""
    cases, prod = {}, {}
    ck = GaussianMixtureConditional(K=4, mode=mode, checkpoint_stride=STRIDE)
    for fam in FAMILIES:
        for lay in F32_LAYOUTS:
            cases[f"{fam}.{lay}.enc"] = _enc_case(*_item(fam, lay))
    for fam in F16_ITEMS:
        for lay in F16_LAYOUTS:
            cases[f"{fam}.{lay}.enc"] = _enc_case(*_item(fam, lay))
    for fam in FAMILIES + F16_ITEMS:  # weights as logits: the reference is fed the device's own softmax
        y, s, m, w = _item(fam)
        prod[f"{fam}.pi_dev"] = _softmax_dev(_logits(w))
        cases[f"{fam}.logits.enc"] = _enc_case(y, s, m, prod[f"{fam}.pi_dev"])
    for name, (y, s, m, w, logits) in _decode_items().items():
        (b, am, zb), _ = ck.compress_batch([dv(y)], [dv(s)], [dv(m)], [dv(w)], weights_are_logits=logits)[0]
        assert am + 1 <= API_DECODE_MAX
        prod[name] = (b, am, zb.cpu())
        pi = prod[f"{name[:-7]}.pi_dev"] if logits else w
        rows = _rows_of(y, _f32(s), _f32(m), _f32(pi), clamp=True)
        cases[f"{name}.ck_enc"] = {"kind": "encode", "v": _ref_quant(y)[2], "s": rows[0], "m": rows[1], "w": rows[2]}
        for sf in E.STREAM_FAMILIES:
            for tag, bb in _streams(sf, b, y.size):
                for bs in sorted({37, am + 1}):
                    cases[f"{name}.{sf}.{tag}.{bs}"] = {"kind": "decode", "bytes": np.frombuffer(bb, np.uint8), "s": rows[0],
                                                        "m": rows[1], "w": rows[2], "max_bs": np.int32(bs)}
    for fam in SEG_TAIL:
        y, s, m, w = _seg_tail_item(fam)
        (b, am, zb), _ = ck.compress_batch([dv(y)], [dv(s)], [dv(m)], [dv(w)])[0]
        prod[f"seg_{fam}"] = (b, am, zb.cpu())
        cases[f"seg_{fam}.enc"] = _enc_case(y, s, m, w)
        for tag, bb in _seg_tail_streams(b):
            cases[f"seg_{fam}.{tag}"] = {**cases[f"seg_{fam}.enc"], "kind": "decode", "bytes": np.frombuffer(bb, np.uint8),
                                         "max_bs": np.int32(am + 1)}
            del cases[f"seg_{fam}.{tag}"]["v"]
    for fam in FAMILIES:  # every edge v - 0.5 of the widest table of the family: the narrower ones are its middle
        wide = fam in E.CLAMP_FAMILIES
        for what, n_t, bs in (("tab", N_TAB, max(TAB_BS)),) + ((("tabw", N_TAB_WIDE, max(TAB_BS_WIDE)),) if wide else ()):
            _, s, m, w = _rows(fam)
            x = (np.arange(-bs, bs + 2).astype(np.float32) - np.float32(0.5)).astype(np.float32)
            rep = lambda a: np.ascontiguousarray(np.repeat(a[:n_t], len(x), 0))  # noqa: E731
            cases[f"{fam}.{what}"] = {"kind": "cdf_x", "x1": np.tile(x, n_t), "x2": np.tile(x, n_t), "s": rep(E.clamp_sigma(s)),
                                      "m": rep(m), "w": rep(w)}
    return cases, prod, W.run(mode, cases, tmp, timeout=1200.0)


@pytest.fixture(scope="module")
def prep(tmp_path_factory):
    assert O.ref_available(), "oracle/_ref is missing: build() makes it and the files travel with the tree"

    def get(mode):
        return _prepared(mode, str(tmp_path_factory.getbasetemp()))

    return get


def _misaligned(a):
    """the tensor as a dense view four bytes (two for float16) into its storage: no 16-byte alignment, so VEC 1"""
    t = dv(a)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    out = buf[1:].view(t.shape)
    assert out.data_ptr() % 16 != 0
    return out


def _same(got, want_bytes, y, what):
    (b, am, zb), yq = got
    am_r, zb_r, _, yq_r = _ref_quant(y)
    assert bytes(b) == want_bytes, f"{what}: bytes differ from the reference's"
    assert am == am_r and zb.cpu().tolist() == zb_r.tolist() and np.array_equal(yq.cpu().numpy(), yq_r), what


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_compress_batch_every_launch_form(prep, ctx_options, mode, fam):
    """the same rows through every form of symtab_kernel<.., CLAMPED = true, ..>: the reference's bytes, abs_max, zero bitmap"""
    _, prod, ref = prep(mode)
    gmc = GaussianMixtureConditional(K=4, mode=mode)

    def want(lay):
        return ref[f"{fam}.{lay}.enc"]["bytes"].tobytes()

    for lay in F32_LAYOUTS:  # linear VEC 4, per-channel VEC 4 (two widths), VEC 1
        y, s, m, w = _item(fam, lay)
        _same(gmc.compress_batch([dv(y)], [dv(s)], [dv(m)], [dv(w)])[0], want(lay), y, lay)
    y, s, m, w = _item(fam)
    t = [dv(a) for a in (y, s, m, w)]
    for opts in ({"enc_vec": 2}, {"enc_linear": 0}, {"enc_vec": 2, "enc_linear": 0}, {"enc_vec": 1}):
        ctx_options(**{"enc_vec": 0, "enc_linear": 1, **opts})
        _same(gmc.compress_batch(*([a] for a in t))[0], want("lin"), y, str(opts))
    ctx_options(enc_vec=0, enc_linear=1)
    mis = [_misaligned(a) for a in (s, m, w)]
    _same(gmc.compress_batch([t[0]], *([a] for a in mis))[0], want("lin"), y, "misaligned planes")
    y2, s2, m2, w2 = _item(fam, "pc4")  # a batch that mixes an aligned and a misaligned item (and two shapes)
    got = gmc.compress_batch([t[0], dv(y2), t[0]], [t[1], dv(s2), mis[0]], [t[2], dv(m2), mis[1]], [t[3], dv(w2), mis[2]])
    for g, lay, yy in zip(got, ("lin", "pc4", "lin"), (y, y2, y)):
        _same(g, want(lay), yy, "mixed batch " + lay)
    lg = dv(_logits(w))
    got = gmc.compress_batch([t[0]], [t[1]], [t[2]], [lg], weights_are_logits=True)[0]
    _same(got, ref[f"{fam}.logits.enc"]["bytes"].tobytes(), y, "logits")
    assert bytes(prod[fam][0]) == ref[f"{fam}.ck_enc"]["bytes"].tobytes() == want("lin")  # the checkpointed stream the decoders get
    ctx_options(enc_segs=2, enc_ways=1)  # segmented tables (forced): M = 9 >= 8, one worker per bitstream
    for g in gmc.compress_batch([t[0], t[0]], [t[1], t[1]], [t[2], t[2]], [t[3], t[3]]):
        _same(g, want("lin"), y, "segmented tables")


@pytest.mark.parametrize("fam", F16_ITEMS)
@pytest.mark.parametrize("mode", MODES)
def test_compress_batch_fp16_launch_forms(prep, ctx_options, mode, fam):
    """float16 planes: VEC 8 linear (hw 512), VEC 8 per channel (hw 256, 64), fp16 VEC 4 (hw 12), misaligned (VEC 1), and the
    narrower loads of option enc_vec on both grids; the reference is fed the widened values"""
    _, prod, ref = prep(mode)
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    for lay in F16_LAYOUTS:
        y, s, m, w = _item(fam, lay)
        assert s.dtype == np.float16
        want = ref[f"{fam}.{lay}.enc"]["bytes"].tobytes()
        _same(gmc.compress_batch([dv(y)], [dv(s)], [dv(m)], [dv(w)])[0], want, y, lay)
        _same(gmc.compress_batch([dv(y)], *([_misaligned(a)] for a in (s, m, w)))[0], want, y, lay + " misaligned")
        if lay == "lin":  # the narrower loads at a shape that takes VEC 8 by default, linear grid and per-channel grid
            for opts in ({"enc_vec": 4}, {"enc_vec": 2}, {"enc_vec": 2, "enc_linear": 0}, {"enc_vec": 4, "enc_linear": 0}):
                ctx_options(**{"enc_linear": 1, **opts})
                _same(gmc.compress_batch([dv(y)], [dv(s)], [dv(m)], [dv(w)])[0], want, y, f"{lay} {opts}")
            ctx_options(enc_vec=0, enc_linear=1)
    y, s, m, w = _item(fam)
    got = gmc.compress_batch([dv(y)], [dv(_f32(s))], [dv(_f32(m))], [dv(_logits(w))], weights_are_logits=True)[0]
    _same(got, ref[f"{fam}.logits.enc"]["bytes"].tobytes(), y, "logits")
    for name in (fam, f"{fam}.logits"):
        assert bytes(prod[name][0]) == ref[f"{name}.ck_enc"]["bytes"].tobytes()


def quant16(c):
    """static_cast<uint16_t>(cdf * 65535) as x86-64 compiles it (cvttss2si, low 16 bits); tests/test_clamped_reference_cpu.py
    holds the oracle's table, which converts with its own code, against the same expression"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (T.torch_int((np.asarray(c, np.float32) * np.float32(65535)).astype(np.float32)).astype(np.int64) & 0xFFFF).astype(np.uint16)


@pytest.mark.parametrize("prune", [1, 0])
@pytest.mark.parametrize("fam,kernel,max_bs", TAB_PARAMS)
@pytest.mark.parametrize("mode", MODES)
def test_tables_equal_the_compiled_reference_entry_for_entry(prep, mode, fam, kernel, max_bs, prune):
    """the virtual table of both table builders with FGMM_TAB_CLAMP, pruned and not: F[v] = quant16(reference cdf at v - 0.5)"""
    _, _, ref = prep(mode)
    wide = max_bs in TAB_BS_WIDE
    what, n_t, big = ("tabw", N_TAB_WIDE, max(TAB_BS_WIDE)) if wide else ("tab", N_TAB, max(TAB_BS))
    full = quant16(ref[f"{fam}.{what}"]["c1"]).reshape(n_t, 2 * big + 2)
    want = full[:, big - max_bs: big - max_bs + 2 * max_bs + 2]
    _, s, m, w = _rows(fam)
    flags = FGMM_TAB_CLAMP | (0 if prune else FGMM_TAB_NO_PRUNE)
    got, _ = gpu_full_table(kernel, mode, s[:n_t], m[:n_t], w[:n_t], max_bs, flags)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (f"{len(bad)} entries differ; first: row {bad[0][0]} v = {bad[0][1] - max_bs}", int(got[tuple(bad[0])]),
                           int(want[tuple(bad[0])]), s[bad[0][0]], m[bad[0][0]], w[bad[0][0]])


@pytest.mark.parametrize("sf", E.STREAM_FAMILIES)
@pytest.mark.parametrize("name", DECODE_ITEMS)
@pytest.mark.parametrize("mode", MODES)
def test_decoders_equal_compiled_reference(prep, ctx_options, mode, name, sf):
    """the product's checkpointed stream and the garbage / truncated / flipped streams derived from it: RansDecoder at two
    max_bs; at the item's own, decompress_batch with the single-pass and the generic table kernel, the host workers and the GPU
    segment decoder - the reference decoder's symbols, a failure exactly where the reference reads past the end"""
    cases, prod, ref = prep(mode)
    b0, am, zb = prod[name]
    y, s, m, w, logits = _decode_items()[name]
    t = [dv(a) for a in (s, m, w)]
    rows = [dv(cases[f"{name}.ck_enc"][k]) for k in ("s", "m", "w")]
    plain = GaussianMixtureConditional(K=4, mode=mode)
    ck = GaussianMixtureConditional(K=4, mode=mode, checkpoint_stride=STRIDE)
    nz = np.nonzero(zb.numpy())[0]
    seg_ok = 2 * (am + 1) + 2 <= 2048  # what the segment decoder takes (fgmm_decode_gpu.cpp)
    assert len(b0.ckpt) == (len(nz) * y.shape[2] * y.shape[3] - 1) // STRIDE >= 7
    cap0 = _lib.get_option(0, "tab_cap_e")
    for tag, bb in _streams(sf, b0, y.size):
        for bs in sorted({37, am + 1}):
            got = _outcome(lambda: ans.RansDecoder().decode_with_indexes_gmm(bb, *rows, bs, mode=mode).numpy())
            _check(got, ref[f"{name}.{sf}.{tag}.{bs}"], f"{name}.{sf}.{tag}.{bs} RansDecoder")
        want = ref[f"{name}.{sf}.{tag}.{am + 1}"]
        if tag == "valid" and name in E.CLAMP_FAMILIES and name != "window_weights":
            assert int(want["past_end"]) == 0 and np.array_equal(want["syms"], _ref_quant(y)[2])

        def as_syms(y_hat):
            return None if y_hat is None else y_hat.cpu().numpy()[0, nz].reshape(-1)

        for what, opts, codec, stream in (("tab", {}, plain, bb), ("generic", {"tab_cap_e": 256}, plain, bb),
                                          ("host workers", {"gpu_decode": 2}, ck, CheckpointedBytes(bb, b0.ckpt, STRIDE)),
                                          ("segment decoder", {"gpu_decode": 1}, ck, CheckpointedBytes(bb, b0.ckpt, STRIDE))):
            ctx_options(**{"tab_cap_e": cap0, "gpu_decode": 0, **opts})
            y_hat = _outcome(lambda: codec.decompress_batch([stream], [am], [zb], [t[0]], [t[1]], [t[2]], weights_are_logits=logits)[0])
            _check(as_syms(y_hat), want, f"{name}.{sf}.{tag} {what}", as_float=True)
            if what == "segment decoder" and y_hat is not None:  # really given to it (decoded there, or handed back)
                assert _lib.ctx_stat(0, 4) + _lib.ctx_stat(0, 5) == int(seg_ok), (name, _lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5))
                if tag == "valid" and name in SEG_SETTLES:
                    assert _lib.ctx_stat(0, 4) == 1, f"{name}: the segment decoder handed a valid stream of monotone rows back"
        ctx_options(gpu_decode=0)
    if name in ("spread_means", WIDE):
        assert not seg_ok and _lib.get_option(0, "tab_cap_e") == cap0
    elif name in E.CLAMP_FAMILIES:
        assert seg_ok


@pytest.mark.parametrize("fam", SEG_TAIL)
@pytest.mark.parametrize("mode", MODES)
def test_segment_decoder_last_segment_equals_compiled_reference(prep, ctx_options, mode, fam):
    """items ordinary up to their last note with the family's rows after it, from the valid stream and from streams whose last
    segment alone is replaced (no note verifies it): the segment decoder, which must hand decreasing rows back, and the table
    path give the reference's symbols"""
    _, prod, ref = prep(mode)
    b, am, zb = prod[f"seg_{fam}"]
    assert bytes(b) == ref[f"seg_{fam}.enc"]["bytes"].tobytes()
    assert zb.tolist() == [1] * LAYOUTS["lin"][0] and len(b.ckpt) == 8 and 2 * (am + 1) + 2 <= 2048
    _, s, m, w = _seg_tail_item(fam)
    t = [dv(a) for a in (s, m, w)]
    ck = GaussianMixtureConditional(K=4, mode=mode, checkpoint_stride=STRIDE)
    for tag, bb in _seg_tail_streams(b):
        want = ref[f"seg_{fam}.{tag}"]
        for how in (1, 2):
            ctx_options(gpu_decode=how)
            y_hat = _outcome(lambda: ck.decompress_batch([CheckpointedBytes(bb, b.ckpt, STRIDE)], [am], [zb], *([a] for a in t))[0])
            _check(None if y_hat is None else y_hat.cpu().numpy().reshape(-1), want, f"seg_{fam}.{tag} gpu_decode={how}", as_float=True)
            if how == 1 and y_hat is not None:
                assert _lib.ctx_stat(0, 4) + _lib.ctx_stat(0, 5) == 1
