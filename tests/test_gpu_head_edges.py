"""GPU (-m gpu): the parameter head kernels (fgmm_head.hip: exact binary32; fgmm_head16.hip: bf16x6) at their edges, against a
float64 reference with the bounds of tests/head_ref.py, the oracle's fmaf chain, and the compiled reference's encoder.

  - a shape grid over M, c_in and hw (ragged channel groups, K tiles, position tiles; both LDS buffers of bf16x6): f32 == the chain
    bit for bit, both arithmetics within their bound of float64, bf16x6 deterministic
  - the head families of tests/edge_corpus.py: f32 == the chain; bf16x6 within its bound, or - features outside its domain - the f32
    head's bits; the IEEE class of float64 wherever the exact result is not finite; weights outside its domain are refused
  - the fused head (compress_head_batch) against the compiled reference: a head W = I fed the concatenated parameter planes of the
    coder's edge families codes the reference's bytes for its own planes, in all modes, both arithmetics, clamp on and off
  - the C ABI with ragged items, uneven offsets, a growing split buffer and misaligned features: each item == its own call"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, ParameterHead, _lib
from oracle import oracle as O
from tests import edge_corpus as E
from tests import head_ref as H
from tests import ref_worker as W_
from tests.test_gpu_reference_edges import API_DECODE_MAX, _decode_inputs, _differ, _ref_quant, _rows_of, _softmax_dev, dv

pytestmark = pytest.mark.gpu
MODES = ["polya", "as", "logistic"]
ARITH = ["f32", "bf16x6"]
DEV = "cuda:0"


def make_head(W, b, arith):
    n_out, c_in = W.shape
    conv = torch.nn.Conv2d(c_in, n_out, 1, bias=b is not None)
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(W.reshape(n_out, c_in, 1, 1)))
        if b is not None:
            conv.bias.copy_(torch.from_numpy(b))
    return ParameterHead(conv.to(DEV), arithmetic=arith)


def head_params(head, x):
    """x [N, c_in, hw] numpy -> [N, 12 M, hw] float32 from the head's un-fused kernel"""
    xt = dv(x[:, :, None, :])
    out = torch.cat(head.params(xt), 1)
    return out[:, :, 0, :].cpu().numpy()


def check_f32(got, W, b, x, what):
    """bit for bit the oracle's chain (a NaN equals any NaN: x86 and the GPU make different default NaNs)"""
    want = O.head_params(W, b, x)
    bad = _differ(got, want)
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], want[bad][:4])


def check_bound(got, W, b, x, bound, what):
    want = H.exact(W, b, x)
    fin = np.isfinite(want)
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(np.float64) - want)
    ok = ~fin | (err <= bound)
    assert ok.all(), (what, int((~ok).sum()), float(np.nanmax(np.where(fin, err / bound, 0))))
    # where the exact result is not finite, the IEEE class of it
    assert np.array_equal(H.ieee_class(got)[~fin], H.ieee_class(want)[~fin]), what
    assert np.isfinite(got[fin]).all(), (what, "a finite exact result came out non-finite")


# ---- the shape grid ------------------------------------------------------------------------------------------------------------
# (M, c_in, hw, N): every M of {1, 15, 16, 17, 33, 192}, c_in of {1, 8, 16, 17, 31, 32, 33, 48, 64, 65, 640, 1040} (odd and even
# numbers of 16-channel tiles) and hw of {1, 3, 4, 31-33, 64, 65, 127-129, 255-257, 300, 513, 1030} at least once
GRID = [(1, 1, 1, 2), (15, 8, 3, 1), (16, 16, 4, 3), (17, 17, 31, 2), (33, 31, 32, 1), (1, 32, 33, 2), (15, 33, 64, 1),
        (16, 48, 65, 2), (17, 64, 127, 1), (33, 65, 128, 2), (192, 640, 129, 1), (1, 1040, 255, 1), (15, 17, 256, 2),
        (16, 33, 257, 1), (17, 65, 300, 2), (33, 8, 513, 1), (1, 31, 1030, 2), (192, 640, 768, 2), (192, 1040, 1030, 1)]


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("M,c_in,hw,N", GRID)
def test_shape_grid(arith, M, c_in, hw, N):
    W, b, _ = E.head_case("ordinary", M, c_in, 1)
    xs = np.stack([E.head_case("ordinary", M, c_in, hw, seed=i + 1)[2] for i in range(N)])
    head = make_head(W, b, arith)
    got = head_params(head, xs)
    bound_of = H.chain_bound if arith == "f32" else H.bf16x6_bound
    for i in range(N):
        check_bound(got[i], W, b, xs[i], bound_of(W, b, xs[i]), (arith, i))
        if arith == "f32":
            check_f32(got[i], W, b, xs[i], i)
    if arith == "bf16x6":
        assert np.array_equal(head_params(head, xs).view(np.uint32), got.view(np.uint32))  # the same bits on a second call


# ---- value families --------------------------------------------------------------------------------------------------------------
FAM_SHAPES = [(17, 33, 65), (15, 65, 257), (1, 17, 300), (16, 1, 4)]


@pytest.mark.parametrize("shape", FAM_SHAPES)
@pytest.mark.parametrize("fam", list(E.HEAD_FAMILIES))
def test_value_families(fam, shape):
    M, c_in, hw = shape
    W, b, x = E.head_case(fam, M, c_in, hw)
    f32 = head_params(make_head(W, b, "f32"), x[None])[0]
    check_f32(f32, W, b, x, fam)
    check_bound(f32, W, b, x, H.chain_bound(*(np.nan_to_num(a) for a in (W, b, x))), fam)
    if fam in E.HEAD_BF16_WEIGHTS_OUT:  # bf16x6: weights whose bfloat16 parts are not finite are refused at creation
        with pytest.raises(RuntimeError):
            make_head(W, b, "bf16x6")
        return
    h16 = make_head(W, b, "bf16x6")
    got = head_params(h16, x[None])[0]
    if fam in E.HEAD_BF16_FEATURES_OUT:  # out of its domain: the item goes to the exact kernel, bit for bit
        assert not H.bf16x6_features_in_domain(x)
        assert not _differ(got, f32).any(), (fam, int(_differ(got, f32).sum()))
    else:
        check_bound(got, W, b, x, H.bf16x6_bound(W, b, x), fam)
    # an item out of the domain beside ordinary ones: only that item changes arithmetic
    x2 = np.stack([E.head_case("ordinary", M, c_in, hw, seed=5)[2], x])
    both = head_params(h16, x2)
    assert not _differ(both[1], got).any()
    check_bound(both[0], W, b, x2[0], H.bf16x6_bound(W, b, x2[0]), (fam, "neighbour"))


# ---- the fused head against the compiled reference -------------------------------------------------------------------------------
FUSED_PARAM = [f for f in E.PARAM_FAMILIES if f not in ("nonfinite_sigma", "nonfinite_mu", "nan_weights")]  # (0 * inf in W = I)
FUSED_CASES = [("p", f) for f in FUSED_PARAM] + [("l", f) for f in E.LATENT_FAMILIES] + [("x", "nonfinite_features")]


def _fused_inputs(kind, fam):
    """-> (y [1, M, h, w], x [1, c_in, h, w], W, b): the identity head over the concatenated planes, or (kind "x") an ordinary head
    whose features hold NaN / +-inf"""
    if kind == "p":
        y, s, m, w = _decode_inputs(fam)
    elif kind == "l":
        y, s, m, w = E.latent_case(fam)
    else:
        y, *_ = E.latent_case("ties_half", h=7, w=15)  # (hw % 4 != 0: the fused kernels' element-wise staging, in every mode)
        M, h, w_ = y.shape[1:]
        W, b, x = E.head_case(fam, M, 40, h * w_)
        return y, x.reshape(1, 40, h, w_), W, b
    W, b = H.identity_head(y.shape[1])
    return y, np.concatenate([s, m, w], 1), W, b


@functools.lru_cache(maxsize=None)
def _fused_prepared(mode, tmp):
    cases, prod = {}, {}
    for kind, fam in FUSED_CASES:
        y, x, W, b = _fused_inputs(kind, fam)
        M = y.shape[1]
        am, zb, sym, yq = _ref_quant(y)
        for arith in ARITH:
            head = make_head(W, b, arith)
            planes = torch.cat(head.params(dv(x)), 1).cpu().numpy()
            s, m, lg = planes[:, : 4 * M], planes[:, 4 * M: 8 * M], planes[:, 8 * M:]
            pi = _softmax_dev(lg)
            for clamp in (True, False):
                gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
                fused = gmc.compress_head_batch(dv(y), dv(x), head)
                plain = gmc.compress_batch([dv(y)], [dv(s)], [dv(m)], [dv(lg)], weights_are_logits=True)
                key = f"{kind}_{fam}.{arith}.{int(clamp)}"
                rows = _rows_of(y, s, m, pi, clamp=clamp)
                cases[key] = {"kind": "encode", "v": sym, "s": rows[0], "m": rows[1], "w": rows[2]}
                dec = None
                if kind == "l" and am + 1 <= API_DECODE_MAX:
                    dec = gmc.decompress_batch(fused.strings, fused.abs_maxes, fused.zero_bitmaps, dv(s), dv(m), dv(lg),
                                               weights_are_logits=True, stacked_output=True).cpu().numpy()
                    # the reference decodes the same stream with the same rows (latents beyond abs_max come back as it says)
                    cases[key + ".dec"] = {"kind": "decode", "bytes": np.frombuffer(bytes(fused.strings[0]), np.uint8), "s": rows[0],
                                           "m": rows[1], "w": rows[2], "max_bs": np.int32(fused.abs_maxes[0] + 1)}
                prod[key] = (fused, plain, dec, planes, (am, zb, yq), x)
    return cases, prod, W_.run(mode, cases, tmp)


@pytest.fixture(scope="module")
def fprep(tmp_path_factory):
    assert O.ref_available(), "oracle/_ref is missing: build() makes it and the files travel with the tree"
    return lambda mode: _fused_prepared(mode, str(tmp_path_factory.getbasetemp()))


@pytest.mark.parametrize("arith", ARITH)
@pytest.mark.parametrize("mode", MODES)
def test_fused_head_equals_compiled_reference(fprep, mode, arith):
    """compress_head_batch: the reference's bytes for the head's own planes (clamped as reshape_entropy_parameters, pi = the
    device's softmax of the logits), abs_max, zero bitmap and y_q of the reference's quantisation; the un-fused path's bytes; the
    identity head gives the planes back (f32: bit for bit, -0 as +0); decode from the head's planes gives y_q"""
    cases, prod, ref = fprep(mode)
    bad = []
    for kind, fam in FUSED_CASES:
        for clamp in (1, 0):
            key = f"{kind}_{fam}.{arith}.{clamp}"
            fused, plain, dec, planes, (am, zb, yq), x = prod[key]
            (bf, af, zf), qf = fused[0]
            (bp, ap, zp), qp = plain[0]
            why = []
            if bytes(bf) != ref[key]["bytes"].tobytes():
                why.append("bytes != reference")
            if bytes(bf) != bytes(bp):
                why.append("bytes != un-fused")
            if not af == am == ap:
                why.append(f"abs_max {af} {ap} != {am}")
            if not zf.tolist() == zb.tolist() == zp.tolist():
                why.append("zero bitmap")
            qf, qp = qf.cpu().numpy().reshape(yq.shape), qp.cpu().numpy().reshape(yq.shape)
            if not (np.array_equal(qf, yq, equal_nan=True) and np.array_equal(qp, yq, equal_nan=True)):
                why.append("y_q")
            if kind != "x":  # W = I gives the planes back: exactly (-0 as +0), but bf16x6 rounds to the bfloat16 subnormal grid
                want = np.where(x == 0, np.float32(0), x)
                off = _differ(planes, want)
                if arith == "bf16x6" and H.bf16x6_features_in_domain(x):
                    off &= ~((np.abs(x) < 2.0**-110) & (np.abs(planes.astype(np.float64) - x) <= 2.0**-133))
                if off.any():
                    why.append(f"planes ({int(off.sum())})")
            if dec is not None:  # the reference decoder's symbols, and y_q when abs_max covers every latent
                nz = np.nonzero(zb.numpy())[0]
                want = ref[key + ".dec"]
                q, got = yq[0, nz].reshape(-1), dec[0, 0, nz].reshape(-1)
                # (with a latent beyond abs_max - NaN, +-inf, |y| >= 2^31 wrap torch's .int() - the reference's own decode drifts)
                covered = np.abs(q) < am if (np.abs(q) < am).all() else np.zeros(q.shape, bool)
                if int(want["past_end"]):
                    why.append("the reference reads past the end")
                if not np.array_equal(got, want["syms"].astype(np.float32)):
                    d = np.nonzero(got != want["syms"].astype(np.float32))[0]
                    why.append(f"decode != reference at {len(d)}: {d[:3]} {got[d[:3]]} {want['syms'][d[:3]]} (y_q {q[d[:3]]})")
                if not np.array_equal(got[covered], q[covered]) or dec[0, 0, np.nonzero(zb.numpy() == 0)[0]].any():
                    why.append("decode != y_q")
            if why:
                bad.append((key, why))
    assert not bad, bad


# ---- the C ABI: ragged items ------------------------------------------------------------------------------------------------------
def _abi_params(head, xptrs, hws):
    L, ctx = _lib.lib(), _lib.ctx(0)
    n = len(hws)
    outs = [torch.full((12 * head.M, max(h, 1)), float("nan"), device=DEV) for h in hws]
    _lib.check(L.fgmm_head_params_batch(ctx, None, head._h, (C.c_void_p * n)(*xptrs), (C.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                        (C.c_int64 * n)(*hws), n), "fgmm_head_params_batch")
    return [o[:, :h].cpu().numpy() for o, h in zip(outs, hws)]


def _abi_fused(head, xptrs, ys, mode=0, clamp=1):
    L, ctx = _lib.lib(), _lib.ctx(0)
    n = len(ys)
    items = (_lib.fgmm_item * n)()
    yq = [torch.empty_like(t) for t in ys]
    zb = [torch.empty(head.M, dtype=torch.int64) for _ in ys]
    for i, t in enumerate(ys):
        items[i].y, items[i].M, items[i].K, items[i].hw = t.data_ptr(), head.M, 4, t.shape[1]
        items[i].yq_out, items[i].zero_bitmap = yq[i].data_ptr(), zb[i].data_ptr()
    _lib.check(L.fgmm_gmc_compress_head_batch(ctx, None, items, (C.c_void_p * n)(*xptrs), n, head._h, mode, clamp),
               "fgmm_gmc_compress_head_batch")
    return [(_lib.take_bytes(items[i].bytes, items[i].bytes_len), items[i].abs_max, zb[i].tolist(), yq[i].cpu().numpy()) for i in range(n)]


@pytest.mark.parametrize("arith", ARITH)
def test_ragged_c_abi(arith):
    M, c_in = 17, 65
    W, b, _ = E.head_case("ordinary", M, c_in, 1)
    head = make_head(W, b, arith)
    rng = np.random.default_rng(3)
    sizes = [300, 0, 35, 1030, 4]
    xs = [E.head_case("ordinary", M, c_in, max(h, 1), seed=i + 1)[2][:, :h] for i, h in enumerate(sizes)]
    ys = [dv((rng.standard_normal((M, h)) * 4).astype(np.float32)) for h in sizes]
    one = [head_params(head, x[None])[0] if x.shape[1] else None for x in xs]
    xt = [dv(x) if x.shape[1] else torch.empty((c_in, 1), device=DEV) for x in xs]  # (alive across the calls that read them)
    one_f = [_abi_fused(head, [t.data_ptr()], [y])[0] for t, y in zip(xt, ys)]

    def same(got_p, got_f, what):
        for i, h in enumerate(sizes):
            if h:
                assert np.array_equal(got_p[i].view(np.uint32), one[i].view(np.uint32)), (what, i)
            assert got_f[i][0] == one_f[i][0] and got_f[i][1:3] == one_f[i][1:3], (what, i)
            assert np.array_equal(got_f[i][3], one_f[i][3]), (what, i)

    # separate allocations
    same(_abi_params(head, [t.data_ptr() for t in xt], sizes), _abi_fused(head, [t.data_ptr() for t in xt], ys), "separate")
    # one tensor at uneven offsets (a float apart from 16-byte alignment)
    offs, at = [], 1
    for x in xs:
        offs.append(at)
        at += x.size + 3
    big = torch.zeros(at, device=DEV)
    for o, x in zip(offs, xs):
        big[o: o + x.size] = dv(x.reshape(-1))
    ptrs = [big.data_ptr() + 4 * o for o in offs]
    same(_abi_params(head, ptrs, sizes), _abi_fused(head, ptrs, ys), "one tensor")
    # small -> large -> small calls on one head (the split buffer grows, then a smaller call reuses it)
    for i in (4, 3, 2):
        got = _abi_params(head, [xt[i].data_ptr()], [sizes[i]])[0]
        assert np.array_equal(got.view(np.uint32), one[i].view(np.uint32)), ("sequence", i)
    # misaligned features at hw % 4 == 0: the element-wise staging (VEC = false) at a size that is otherwise vectorised
    x = xs[0][:, :296]
    mis = torch.zeros(x.size + 1, device=DEV)
    mis[1:] = dv(x.reshape(-1))
    got = _abi_params(head, [mis.data_ptr() + 4], [296])[0]
    want = head_params(head, np.ascontiguousarray(x)[None])[0]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if arith == "f32":
        check_f32(got, W, b, np.ascontiguousarray(x), "misaligned")
    y, xa = ys[0][:, :296].contiguous(), dv(np.ascontiguousarray(x))
    assert _abi_fused(head, [mis.data_ptr() + 4], [y])[0][:3] == _abi_fused(head, [xa.data_ptr()], [y])[0][:3]
