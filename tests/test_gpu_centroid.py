"""GPU (-m gpu): centroid reconstruction of decoded latents (include/flashgmm_amd.h section 3i; centroid_kernel in fgmm_centroid.hip,
fgmm_centroid.cpp) - through the C entry point, ``GaussianMixtureConditional.reconstruct / reconstruct_batch`` and the latent codecs'
``centroid=True``.

Yardsticks, named per test:
  accuracy     E_k <= 2 * E_ref + 2^-23 against the float64 closed form (tests/centroid_ref.py, no series), the rule of
               tests/test_gpu_likelihood.py applied to the ABSOLUTE error of off = rec - v, per region; E_ref is the header's binary32
               sequence evaluated by torch on the GPU.  Every figure is printed before it is asserted (run with -s).
  decision     outside ``near`` rows (float64 L within 1e-3 of p_min, |off| within 1e-3 of 1/2; at most 1 % may be excluded) keep is the
               float64 decision exactly; a dropped row's rec is v bit for bit; n_kept counts the kernel's own kept rows.
  relayout     a call on another layout, alignment, plane type or batch equals the plain call - dense, aligned float32 planes holding the
               widened values, one item - bit for bit.  Each case asserts its launch form (tests/like_ref.py, CASES) first.
  equivalence  the logits form equals the plain call on the planes fgmm_softmax4_hip makes of the logits, bit for bit."""
import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, _lib
from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec, CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec
from test_gpu_likelihood import DEV, _fill, dv, make
from test_gpu_likelihood_edges import DT, assert_form, fitem, off, one, same
from test_gpu_likelihood_logits import SHAPES, make_l, softmax4_planes
from test_gpu_streams import delay, pending, snapshot, streams  # noqa: F401  (the stream case runs in that module's manner, on its helpers)
from test_likelihood_logits_cpu import INSTANTIATION_CASES
from tests import centroid_ref as Z
from tests import like_logits_ref as Q
from tests import like_ref as R
from tests import synth as T

pytestmark = pytest.mark.gpu

F32 = torch.float32
LOGITS = _lib.FGMM_PARAMS_LOGITS
NAN_FILL = 0x7FC0BEEF  # the pattern rec is pre-filled with where a test watches what is written


def patterned(shape):
    return torch.full(tuple(shape), NAN_FILL, dtype=torch.int32, device=DEV).view(F32)


def untouched(t):
    return bool(torch.all(t.view(torch.int32) == NAN_FILL))


def raw(items, logits=False, sb=R.SB, p_min=Z.P_MIN, K=4, flags=None, recs=None, sizes=None):
    """fgmm_gmc_centroid_batch on items (y [M, h, w], scales, means, weights [4M, h, w]) on the current stream -> (rc, [(rec, n_kept)]);
    ``recs``: per item the caller's rec (default: a fresh one holding the NaN pattern); ``sizes``: per item (M, hw) in place of the
    tensors' own; ``flags``: one value or one per item in place of the form's own"""
    arr = (_lib.fgmm_centroid_item * len(items))()
    outs = []
    for i, (it, (y, s, m, w)) in enumerate(zip(arr, items)):
        fl = (LOGITS if logits else 0) if flags is None else flags[i] if isinstance(flags, (list, tuple)) else flags
        _fill(it, y, s, m, w, K, fl, sizes[i] if sizes else None)
        rec = recs[i] if recs is not None else patterned(y.shape)
        it.rec = None if rec is None else rec.data_ptr()
        outs.append(rec)
    torch.cuda.current_stream().synchronize()
    rc = _lib.lib().fgmm_gmc_centroid_batch(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, arr, len(items), sb, p_min)
    return rc, [(rec, int(it.n_kept)) for it, rec in zip(arr, outs)]


def plain(item, **kw):
    """the plain call of one item: fresh, dense, aligned float32 tensors holding the widened values, alone"""
    item = tuple(t.to(F32).clone() for t in item)
    assert all(t.data_ptr() % 16 == 0 for t in item)
    rc, [res] = raw([item], **kw)
    assert rc == 0
    return res


def check_relayout(items, res, what, sizes=None, **kw):
    for i, (item, (rec, n)) in enumerate(zip(items, res)):
        if sizes is not None and sizes[i][0] * sizes[i][1] == 0:
            assert n == 0 and untouched(rec), (what, i)
            continue
        want, want_n = plain(item, **kw)
        assert same(rec, want) and n == want_n, (what, i)


# ---- 1. the kernel against float64 on the corpus ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def corpus_ref():
    """computed once per plane type, left unchanged: the corpus with its planes rounded to the type, the float64 closed form of the widened
    values and the header's binary32 sequence by torch on the GPU"""
    out = {}
    for dt in R.ALL:
        cpu = [torch.from_numpy(a) for a in R.corpus()[:4]]
        cpu = [cpu[0]] + [t.to(DT[dt]) for t in cpu[1:]]
        gpu = [t.to(DEV) for t in cpu]
        wide = [t.to(F32) for t in cpu]
        out[dt] = dict(gpu=gpu, c64=Z.centroid(*wide, dtype=torch.float64, form="closed"), c32=Z.centroid(*(t.to(F32) for t in gpu)))
    return out


@pytest.mark.parametrize("dt", R.ALL)
def test_kernel_against_float64_on_the_corpus(corpus_ref, dt):
    """accuracy and decision, per region, float32 / float16 / bfloat16 planes"""
    ref = corpus_ref[dt]
    item = tuple(t[0] for t in ref["gpu"])
    rec = patterned(item[0].shape)
    assert R.launch_form([fitem(*item, rest=[rec])], dt != "f32", False) == (4, R.LIN)  # (M 8, hw 256: two-byte planes give up 8 for the linear grid)
    rc, [(rec, n_kept)] = raw([item], recs=[rec])
    assert rc == 0
    c64, c32 = ref["c64"], ref["c32"]
    v = c64["v"].reshape(-1).numpy()
    rec_k = rec.reshape(-1).cpu().numpy()
    rec_32, keep_32 = c32["rec"].reshape(-1).cpu().numpy(), c32["keep"].reshape(-1).cpu().numpy()
    off_64, keep_64 = c64["off"].reshape(-1).numpy(), c64["keep"].reshape(-1).numpy()
    nr = Z.near(c64["L"].reshape(-1).numpy(), off_64)
    print(f"[{dt}] near rows {int(nr.sum())} of 2048; kept by float64 {int(keep_64.sum())}, n_kept {n_kept}")
    assert nr.mean() <= 0.01
    # decision: a row the kernel moved is a row float64 keeps; a row float64 drops comes back as v, bit for bit
    moved = rec_k != v.astype(np.float32)
    assert not np.any(moved & ~keep_64 & ~nr)
    dropped = ~keep_64 & ~nr
    assert np.array_equal(rec_k[dropped].view(np.int32), v.astype(np.float32)[dropped].view(np.int32))
    # a kept row whose offset is below half an ulp of v stays at v: counted from the restatement (the kernel's keep is not an output)
    silent = ~moved & keep_32 & (rec_32 == v.astype(np.float32))
    assert np.array_equal((moved | silent)[~nr], keep_64[~nr])
    assert n_kept == int(moved.sum() + silent.sum())
    # accuracy of off = rec - v on the rows float64 keeps
    for name, (lo, hi) in R.REGIONS.items():
        rows = np.zeros(2048, bool)
        rows[lo:hi] = True
        rows &= keep_64 & keep_32 & ~nr
        if not rows.any():
            assert name == "c"
            continue
        e = lambda x: float(np.abs((x.astype(np.float64) - v) - off_64)[rows].max())  # noqa: E731
        e_ref, e_k = e(rec_32), e(rec_k)
        print(f"accuracy [{dt}] off ({name}) {int(rows.sum()):3d} rows  E_ref {e_ref:.3e}  E_k {e_k:.3e}  ratio {e_k / e_ref if e_ref else float('inf') if e_k else 1.0:.3f}")
        assert e_k <= 2.0 * e_ref + 2.0 ** -23, (dt, name, e_ref, e_k)


# ---- 2. every launch form -----------------------------------------------------------------------------------------------------------------
def case_items(case, dt):
    """-> (items, sizes) of a case of R.CASES, laid out as the case says (tests/test_gpu_likelihood_logits.py lays its logits out the same)"""
    items = [one(8100 + 10 * len(case) + i, *shp, dt)[0] for i, shp in enumerate(SHAPES[case])]
    sizes = None
    if case == "old_offset_hw256":
        items = [tuple(off(t, 4) for t in it) for it in items]
    elif case == "a_planes_off":
        items = [(it[0],) + tuple(off(t, 2) for t in it[1:]) for it in items]
    elif case in ("b_M0", "b_hw0"):
        sizes = [(0, 256) if case == "b_M0" else (2, 0), (2, 256)]
    elif case.startswith("c_chunk"):  # strided planes: the chunk views of a [2, 12M, h, w] tensor, what a parameter network's output gives
        M, h, w = SHAPES[case][0]
        views = items[0][1].new_empty((2, 12 * M, h, w)).chunk(3, 1)
        for i, it in enumerate(items):
            for vw, t in zip(views, it[1:]):
                vw[i].copy_(t)
        assert not any(vw.is_contiguous() for vw in views)
        items = [(it[0],) + tuple(vw[i] for vw in views) for i, it in enumerate(items)]
    return items, sizes


@pytest.mark.parametrize("case,dt", INSTANTIATION_CASES)
def test_every_launch_form(case, dt):
    """relayout, on the forward launch forms of R.CASES - VEC 1 / 4 / 8 in both grids, planes a few to about 260 positions, misaligned by
    one element, strided, unequal and empty items (tests/test_centroid_cpu.py: together they are all 16 forward forms)"""
    items, sizes = case_items(case, dt)
    recs = [patterned(it[0].shape) if case != "old_offset_hw256" else off(patterned(it[0].shape), 4) for it in items]
    assert_form(case, dt, [fitem(*it, rest=[r], size=sizes[i] if sizes else None) for i, (it, r) in enumerate(zip(items, recs))], False)
    rc, res = raw(items, recs=recs, sizes=sizes)
    assert rc == 0
    check_relayout(items, res, (case, dt), sizes)


# ---- 3. logits ------------------------------------------------------------------------------------------------------------------------------
def plain_of(item):
    y, s, m, lg = item
    return (y, s.to(F32), m.to(F32), softmax4_planes(lg))


def test_logits_form_equals_the_plain_call_on_the_corpus():
    """equivalence on the logits corpus, and on planted non-finite logits, where softmax4 decides as in section 3h: a +inf logit or four
    of -inf give NaN weights and rec == v; a NaN or a -inf logit is a component of weight 0, and the row is the plain call's on those
    weights like every other"""
    y, s, m, lg = (dv(a)[0] for a in Q.logits_corpus()[:4])
    rc, [(rec, n)] = raw([(y, s, m, lg)], logits=True)
    want, want_n = plain(plain_of((y, s, m, lg)))
    assert rc == 0 and same(rec, want) and n == want_n and n > 1000
    arrays = Q.nonfinite_logits()
    y, s, m, lg = (dv(a)[0] for a in arrays[:4])
    rc, [(rec, n)] = raw([(y, s, m, lg)], logits=True)
    item = plain_of((y, s, m, lg))
    want, want_n = plain(item)
    assert rc == 0 and same(rec, want) and n == want_n
    flat_rec, v, P = rec.reshape(-1), torch.round(y).reshape(-1), item[3].reshape(4, -1)
    for kind, i, k in arrays[5]:
        if kind in ("pinf", "all_ninf"):
            assert bool(torch.isnan(P[:, i]).all()) and same(flat_rec[i], v[i]), (kind, i)
        else:
            assert float(P[k, i]) == 0.0 and bool(torch.isfinite(P[:, i]).all()), (kind, i)
    assert sum(bool(flat_rec[i] != v[i]) for kind, i, _ in arrays[5] if kind in ("nan", "ninf")) >= 4  # (three components still say where)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (1, 4, 16, 16), (2, 2, 16, 32)])  # 1, 4 and 8 positions per lane
def test_two_byte_logits_equal_the_plain_call_on_the_widened_values(dt, shape):
    y, s, m, lg, _ = make_l(8300 + shape[2], *shape, dtype=DT[dt])
    items = [(y[i], s[i], m[i], lg[i]) for i in range(shape[0])]
    recs = [patterned(it[0].shape) for it in items]
    vec = {35: 1, 256: 4, 512: 8}[shape[2] * shape[3]]
    assert R.launch_form([fitem(*it, rest=[r]) for it, r in zip(items, recs)], True, False)[0] == vec
    rc, res = raw(items, logits=True, recs=recs)
    assert rc == 0
    check_relayout([plain_of(it) for it in items], res, (dt, shape))


# ---- 4. non-finite inputs -------------------------------------------------------------------------------------------------------------------
def test_non_finite_inputs_keep_v_and_disturb_nothing_else():
    """classes: NaN / inf sigma, weight or mean -> rec == v; a non-finite y comes back as it is; a zero sigma is the scale bound's; every
    other row equals the clean corpus's; nothing is written outside rec (guard elements either side, NaN pattern)"""
    arrays = R.edge_inputs()
    y, s, m, w = (dv(a)[0] for a in arrays[:4])
    clean = [dv(a)[0] for a in R.corpus()[:4]]
    buf = patterned((y.numel() + 64,))
    rec = buf[32:-32].view(y.shape)
    rc, [(_, n)] = raw([(y, s, m, w)], recs=[rec])
    assert rc == 0 and untouched(buf[:32]) and untouched(buf[-32:])
    want, want_n = plain(tuple(clean))
    hole = torch.from_numpy(R.planted_mask(arrays[5])[0]).to(DEV)
    assert same(rec[~hole], want[~hole])
    flat_rec, flat_y = rec.reshape(-1), y.reshape(-1)
    s_fix = s.clone()
    s_fix[s_fix == 0] = R.f32(R.SB)
    fixed = plain((clean[0], s_fix, clean[2], clean[3]))[0].reshape(-1)
    for kind, i, k in arrays[5]:
        if kind == "sigma_zero":
            assert same(flat_rec[i], fixed[i]), (kind, i)
        elif kind in ("y_pinf", "y_ninf", "y_mu_pinf"):
            assert same(flat_rec[i], flat_y[i]), (kind, i)
        else:
            assert same(flat_rec[i], torch.round(flat_y[i])), (kind, i)
    assert want_n - len(arrays[5]) <= n <= want_n + 8  # (the other planted rows can only leave the count, the 8 zero sigmas may join it)


# ---- 5. batches ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_a_batch_of_unequal_items_with_an_empty_one_and_rec_over_y(dt):
    """relayout: unequal items, an empty one between them, and every rec the item's own y"""
    shapes = [(2, 16, 16), (5, 16, 16), (3, 5, 7), (1, 16, 32)]
    items = [one(8500 + i, *shp, dt)[0] for i, shp in enumerate(shapes)]
    sizes = [(2, 256), (0, 256), (3, 35), (1, 512)]
    keep_y = [it[0].clone() for it in items]
    rc, res = raw(items, recs=[it[0] for it in items], sizes=sizes)
    assert rc == 0 and res[1][1] == 0 and same(items[1][0], keep_y[1])  # (the empty item: nothing written)
    for i in (0, 2, 3):
        want, want_n = plain((keep_y[i],) + items[i][1:])
        assert same(res[i][0], want) and res[i][1] == want_n and res[i][0].data_ptr() == items[i][0].data_ptr(), i


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    y, s, m, w, _ = make(8600, 2, 4, 8, 8)
    items = [(y[i], s[i], m[i], w[i]) for i in range(2)]
    bad = (dict(K=3), dict(flags=2), dict(flags=LOGITS | 2), dict(flags=[0, LOGITS]), dict(flags=[LOGITS, 0]), dict(sb=0.0), dict(sb=-1.0),
           dict(sb=float("inf")), dict(sb=float("nan")), dict(p_min=0.0), dict(p_min=-1.0), dict(p_min=float("inf")), dict(p_min=float("nan")))
    for kw in bad:
        rc, res = raw(items, **kw)
        torch.cuda.synchronize()
        assert rc == 1 and all(untouched(rec) for rec, _ in res), kw
    full = patterned(y[0].shape)
    rc, _ = raw(items, recs=[full, None])  # a null rec in the second item
    torch.cuda.synchronize()
    assert rc == 1 and untouched(full)
    arr = (_lib.fgmm_centroid_item * 1)()
    _fill(arr[0], *items[0])
    arr[0].y, arr[0].rec = None, full.data_ptr()  # a null y
    assert _lib.lib().fgmm_gmc_centroid_batch(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, arr, 1, R.SB, Z.P_MIN) == 1 and untouched(full)
    assert raw(items)[0] == 0 and raw(items, logits=True)[0] == 0  # (the same items are taken as they are, in either form)


# ---- 7. the caller's-stream contract --------------------------------------------------------------------------------------------------------------
def test_centroid_with_a_pending_producer(streams, delay):  # noqa: F811
    s1, _, third = streams
    true, decoy = make(8700, 2, 4, 16, 16)[:4], make(8701, 2, 4, 16, 16)[:4]
    split = lambda t: [tuple(x[i] for x in t) for i in range(2)]  # noqa: E731
    rc, want = raw(split(true))
    assert rc == 0 and not torch.equal(want[0][0], raw(split(decoy))[1][0][0])
    with pending(s1, delay, true, decoy) as t:
        rc, res = raw(split(t))
        seen = snapshot(third, [r for r, _ in res])
    assert rc == 0 and all(same(a, b[0]) for a, b in zip(seen, want)) and [n for _, n in res] == [n for _, n in want]


# ---- 8. the benefit ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_lowers_the_squared_error_on_sampled_latents():
    """latents drawn from their own mixtures (M = 4, 32 x 32): the kernel's rec, given round(y) as a decoder would be, has a lower mean
    squared error than rounding, within 1e-4 relative of the float64 centroid's"""
    arrays = Z.sample()
    y = arrays[0].astype(np.float64)
    c64 = Z.centroid(*(torch.from_numpy(a) for a in arrays), dtype=torch.float64, form="closed")
    gmc = GaussianMixtureConditional(K=4)
    y_hat = torch.round(dv(arrays[0]))
    rec, n_kept = gmc.reconstruct(y_hat, *(dv(a) for a in arrays[1:]), return_kept=True)
    assert rec.shape == y_hat.shape and rec.dtype == F32 and int((rec != y_hat).sum()) <= n_kept <= y.size
    e_round, e_64 = float(np.mean((y - np.round(y)) ** 2)), float(np.mean((y - c64["rec"].numpy()) ** 2))
    e_k = float(np.mean((y - rec.cpu().numpy().astype(np.float64)) ** 2))
    print(f"mean squared latent error: rounding {e_round:.5f}, float64 centroid {e_64:.5f}, kernel {e_k:.5f} (relative to float64 {e_k / e_64 - 1:+.2e}), kept {n_kept} of {y.size}")
    assert e_k < e_round and abs(e_k / e_64 - 1.0) <= 1e-4


# ---- 9. the Python surface and the codecs -------------------------------------------------------------------------------------------------------------
def test_reconstruct_and_reconstruct_batch():
    gmc = GaussianMixtureConditional(K=4)
    y, s, m, w, _ = make(8800, 3, 3, 8, 8, dtype=torch.bfloat16)
    y_hat = torch.round(y)
    items = [(y_hat[i], s[i], m[i], w[i]) for i in range(3)]
    rc, want = raw(items)
    assert rc == 0
    stacked = gmc.reconstruct_batch(y_hat, s, m, w, return_kept=True)
    listed = gmc.reconstruct_batch([y_hat[i:i + 1] for i in range(3)], *([t[i:i + 1] for i in range(3)] for t in (s, m, w)))
    for i in range(3):
        assert same(stacked[i][0], want[i][0][None]) and stacked[i][1] == want[i][1] and same(listed[i], want[i][0][None])
    single = gmc.reconstruct(y_hat[:1].requires_grad_(True), s[:1], m[:1], w[:1])
    assert same(single, want[0][0][None]) and not single.requires_grad
    lg = make_l(8801, 1, 3, 8, 8)[3]
    rec = gmc.reconstruct(y_hat[:1], s[:1].to(F32), m[:1].to(F32), lg, weights_are_logits=True, p_min=2.0 ** -10)
    assert same(rec, raw([(y_hat[0], s[0].to(F32), m[0].to(F32), lg[0])], logits=True, p_min=2.0 ** -10)[1][0][0][None])
    assert gmc.reconstruct_batch([], [], [], []) == []


def ckbd(c, c_side, centroid, **kw):
    Ctx, Par = T.exact_modules()
    inner = GaussianMixtureConditionalLatentCodec(K=4, mode="polya", centroid=centroid, **kw)
    return CheckerboardLatentCodec(latent_codec={"y": inner}, context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c)).cuda()


def halves_rec(codec, strings, shape, side):
    """The "y_rec" rebuilt half by half from the public pieces: the halves' parameters as decompress forms them (the context from y_hat), the
    planes the coder was given, the entropy model's decompress and reconstruct"""
    c, h, w = shape
    inner = codec.latent_codec["y"]
    gmc = inner.gaussian_mixture_conditional
    y_hat_ = side.new_zeros((2, 1, c, h, w // 2))
    y_rec_ = torch.zeros_like(y_hat_)
    side_ = codec.unembed(side)
    for i in range(2):
        sc, me, wt = inner._params(codec.entropy_parameters(codec.merge(codec._ctx(y_hat_, i), side_[i])))
        add = None
        if inner.quantizer != "noise":
            add, me = inner._recentre(me, wt)
        planes = inner._planes(sc, me, wt)
        decoded = gmc.decompress(*strings[i], *planes, weights_are_logits=inner.fuse_softmax)
        rec = gmc.reconstruct(decoded, *planes, weights_are_logits=inner.fuse_softmax, p_min=inner.centroid_p_min)
        y_hat_[i], y_rec_[i] = (decoded, rec) if add is None else (decoded + add, rec + add)
    return codec.embed(y_hat_), codec.embed(y_rec_)


@pytest.mark.parametrize("kw", [dict(), dict(quantizer="weighted_mean_ste"), dict(fuse_softmax=True), dict(param_dtype=torch.bfloat16)], ids=lambda kw: "-".join(kw) or "plain")
def test_checkerboard_codec_with_centroid(kw):
    """M = 8, 8 x 8, the exact 1x1 networks of tests/synth.py: y_hat is bit for bit what it is with the option off, y_rec the halves'
    reconstruct, embedded; the same through decompress_many"""
    c, c_side, h, w = 8, 8, 8, 8
    on, off_ = ckbd(c, c_side, True, **kw), ckbd(c, c_side, False, **kw)
    data = [[dv(a) for a in T.exact_codec_inputs(8900 + i, c, c_side, h, w)] for i in range(2)]
    encs = [off_.compress(y, side) for y, side in data]
    for (y, side), enc in zip(data, encs):
        a, b = on.decompress(enc["strings"], enc["shape"], side), off_.decompress(enc["strings"], enc["shape"], side)
        assert set(b) == {"y_hat"} and set(a) == {"y_hat", "y_rec"}
        want_hat, want_rec = halves_rec(on, enc["strings"], enc["shape"], side)
        assert same(a["y_hat"], b["y_hat"]) and same(a["y_hat"], want_hat) and same(a["y_rec"], want_rec)
        assert bool((a["y_rec"] != a["y_hat"]).any()) and float((a["y_rec"] - a["y_hat"]).abs().max()) <= 0.5 + 2.0 ** -16  # (a few ulps of |y| < 64)
    many_on = on.decompress_many([e["strings"] for e in encs], encs[0]["shape"], [side for _, side in data])
    many_off = off_.decompress_many([e["strings"] for e in encs], encs[0]["shape"], [side for _, side in data])
    for (y, side), enc, a, b in zip(data, encs, many_on, many_off):
        assert set(b) == {"y_hat"} and same(a["y_hat"], b["y_hat"]) and same(a["y_rec"], on.decompress(enc["strings"], enc["shape"], side)["y_rec"])


def test_channel_groups_codec_concatenates():
    Ctx, Par = T.exact_modules()
    groups, c_side, h, w = [2, 2, 4], 8, 8, 8
    c = sum(groups)

    def build(centroid):
        gmm = lambda: GaussianMixtureConditionalLatentCodec(K=4, mode="polya", centroid=centroid)  # noqa: E731
        latent = {f"y{k}": CheckerboardLatentCodec(latent_codec={"y": gmm()}, context_prediction=Ctx(g, 2 * g),
                                                   entropy_parameters=Par(2 * g + (k > 0) * 2 * g + c_side, g)) for k, g in enumerate(groups)}
        chctx = {f"y{k}": Ctx(sum(groups[:k]), 2 * groups[k]) for k in range(1, len(groups))}
        return ChannelGroupsLatentCodec(groups=groups, channel_context=chctx, latent_codec=latent).cuda()

    on, off_ = build(True), build(False)
    y, side = (dv(a) for a in T.exact_codec_inputs(9000, c, c_side, h, w))
    enc = off_.compress(y, side)
    a, b = on.decompress(enc["strings"], enc["shape"], side), off_.decompress(enc["strings"], enc["shape"], side)
    assert set(b) == {"y_hat"} and set(a) == {"y_hat", "y_rec"} and same(a["y_hat"], b["y_hat"]) and torch.equal(a["y_hat"], enc["y_hat"])
    # group k's y_rec is its checkerboard codec's, under the channel context of the y_hat of the groups before
    views = a["y_hat"].split(groups, dim=1)
    per = len(enc["strings"]) // len(groups)
    parts = [on.latent_codec[f"y{k}"].decompress(enc["strings"][per * k: per * (k + 1)], enc["shape"][k], on._get_ctx_params(k, side, views))["y_rec"]
             for k in range(len(groups))]
    assert same(a["y_rec"], torch.cat(parts, 1)) and bool((a["y_rec"] != a["y_hat"]).any())
    (m,) = on.decompress_many([enc["strings"]], enc["shape"], [side])
    assert same(m["y_hat"], a["y_hat"]) and same(m["y_rec"], a["y_rec"])
