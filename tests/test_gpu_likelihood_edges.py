"""GPU (-m gpu): the likelihood kernels (include/flashgmm_amd.h section 3g; fgmm_like.hip, fgmm_like.cpp) where tests/test_gpu_likelihood.py
does not go - every instantiation the launcher's ladder can pick, its batch-wide decisions on unequal items, strided planes, partial
outputs, bounds other than the defaults, the g_bits path on the whole corpus, non-finite inputs.

No tolerance of its own.  Three yardsticks, named per test:
  relayout   a call on another layout, alignment, batch composition or subset of outputs equals the plain call - dense, aligned, one
             item, every output - on the same values, bit for bit;
  accuracy   distinct values: E_k <= 2 * E_ref + 2^-23 against float64 (R.forward / R.reference_gradients), through check_accuracy of
             tests/test_gpu_likelihood.py;
  classes    NaN, +inf, -inf, zero, other finite: per element the class of the float32 restatement on the GPU (R.forward / R.backward).
Every case names the launch form it is there for (tests/like_ref.py, CASES) and asserts it on the addresses it really passes, through
R.launch_form, before the call: a case that silently lands on another kernel fails.  tests/test_likelihood_cpu.py holds the table to
the union of all 28 instantiations."""
import itertools

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional
from test_gpu_likelihood import DEV, check_accuracy, dv, grads_through_map, make, raw_backward, raw_forward
from tests import like_ref as R

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
GB = (1.5, -0.375, 0.75)


@pytest.fixture(scope="module")
def gmc():
    return GaussianMixtureConditional(K=4).eval()


def same(a, b):
    """bit for bit (NaN equals NaN, 0 differs from -0)"""
    if a is None or b is None:
        return a is None and b is None
    ints = {4: torch.int32, 2: torch.int16}
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(ints[a.element_size()]), b.contiguous().view(ints[b.element_size()]))


def off(t, nbytes=4):
    """the same values `nbytes` past a 16-byte boundary"""
    n = nbytes // t.element_size()
    r = t.new_empty(t.numel() + n)[n:].view(t.shape).copy_(t)
    assert r.data_ptr() % 16 == nbytes
    return r


def fitem(y, s, m, w, rest=(), size=None):
    """a ctypes item's tensors (and the call's other pointers) as R.launch_form reads them"""
    M, hw = size if size is not None else (y.shape[0], y[0].numel())
    return R.form_item(hw, hw, M * hw, [t.data_ptr() for t in (s, m, w)], [y.data_ptr()] + [0 if t is None else t.data_ptr() for t in rest])


def assert_form(name, dt, items, backward):
    got = R.launch_form(items, dt != "f32", backward)
    assert got == R.FORMS[name, dt][int(backward)], (name, dt, backward, got)


def one(seed, M, h, w, dt):
    """one ctypes item of typical values -> ((y, scales, means, weights), g)"""
    t = make(seed, 1, M, h, w, dtype=DT[dt])
    return tuple(x[0] for x in t[:4]), t[4][0]


def all_same(xs, ys):
    return len(xs) == len(ys) and all(same(a, b) for a, b in zip(xs, ys))


# ---- a. two-byte planes at one position per lane, on either grid ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", ["a_hw35", "a_planes_off", "a_y_off"])
def test_two_byte_planes_one_position_per_lane(gmc, dt, case):
    """relayout (and accuracy at hw 35): EncPlanes<_Float16, 1> and EncPlanes<__bf16, 1>, forward and backward - odd hw on the tiled grid;
    planes 2 bytes off on the linear grid; aligned planes that would allow 4 per lane but a latent 4 bytes off.  Each equals the call
    on aligned float32 planes holding the widened values."""
    B, M, h, w = {"a_hw35": (1, 3, 5, 7), "a_planes_off": (2, 3, 8, 8), "a_y_off": (1, 4, 16, 16)}[case]
    y, s, m, wt, g = make(5100 + len(case), B, M, h, w, dtype=DT[dt])
    wide, y_plain = [x.to(torch.float32) for x in (s, m, wt)], y
    if case == "a_planes_off":
        s, m, wt = (off(x, 2) for x in (s, m, wt))
    if case == "a_y_off":
        y = off(y, 4)
    items2 = [(y[i], s[i], m[i], wt[i]) for i in range(B)]
    items4 = [(y_plain[i], wide[0][i], wide[1][i], wide[2][i]) for i in range(B)]
    for back in (False, True):
        assert_form(case, dt, [fitem(*it) for it in items2], back)
    for rnd in (True, False):
        v2, like2, grads2 = grads_through_map(gmc, y, s, m, wt, g, rnd)
        v4, like4, grads4 = grads_through_map(gmc, y_plain, *wide, g, rnd)
        assert same(v2, v4) and same(like2, like4)
        for name, a, b in zip(R.GRADS, grads2, grads4):
            assert (a is None) == (b is None) == (rnd and name == "dy")
            if a is not None:
                assert a.dtype == (DT[dt] if name != "dy" else torch.float32) and same(a, b.to(a.dtype)), (name, rnd)
        (rc2, f2), (rc4, f4) = raw_forward(items2, rnd), raw_forward(items4, rnd)
        assert rc2 == 0 and rc4 == 0
        for (l2, w2, b2, n2), (l4, w4, b4, n4) in zip(f2, f4):
            assert same(l2, l4) and same(w2, w4) and b2 == b4 and n2 == n4 == 0
        for gs, gb in ((list(g), None), (None, list(GB[:B]))):
            (rc2, o2), (rc4, o4) = raw_backward(items2, gs, rnd, g_bits=gb), raw_backward(items4, gs, rnd, g_bits=gb)
            assert rc2 == 0 and rc4 == 0 and all(all_same(a, b) for a, b in zip(o2, o4)), (rnd, gb)
    if case == "a_hw35":
        cpu = [y.cpu()] + [x.cpu() for x in wide] + [g.cpu()]
        for rnd in (True, False):
            f64, f32 = R.forward(*cpu[:4], rnd=rnd, dtype=torch.float64), R.forward(y, *wide, rnd=rnd)
            _, like, grads = grads_through_map(gmc, y, *wide, g, rnd)  # (== the two-byte call's, bit for bit: above)
            check_accuracy(f"{dt} hw35 likelihood rnd={int(rnd)}", like.cpu().numpy(), f32["out"].cpu().numpy(), f64["out"].numpy(), floor=R.f32(R.LB))
            b64, b32 = R.reference_gradients(*cpu, rnd=rnd)[1], R.backward(f32, g)
            for name, got in zip(R.GRADS, grads):
                if got is not None:
                    check_accuracy(f"{dt} hw35 {name} rnd={int(rnd)}", got.cpu().numpy(), b32[name].cpu().numpy(), b64[name].numpy())


# ---- b. batches through ctypes ------------------------------------------------------------------------------------------------------------
def plain_calls(item, g, gb, rnd, **kw):
    """the plain call of one item: dense, aligned, alone, every output -> (forward's tuple, backward at g, backward at g_bits)"""
    item = tuple(t.clone() for t in item)
    assert all(t.data_ptr() % 16 == 0 for t in item)
    (rc1, [f]), (rc2, [b]), (rc3, [bb]) = raw_forward([item], rnd, **kw), raw_backward([item], [g.clone()], rnd, **kw), raw_backward([item], None, rnd, g_bits=[gb], **kw)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    return f, b, bb


def check_batch(name, dt, items, gs):
    for back in (False, True):
        assert_form(name, dt, [fitem(*it, rest=() if not back else (g,)) for it, g in zip(items, gs)], back)
    gbs = list(GB[:len(items)])
    for rnd in (True, False):
        (rc1, f), (rc2, b), (rc3, bb) = raw_forward(items, rnd), raw_backward(items, gs, rnd), raw_backward(items, None, rnd, g_bits=gbs)
        assert rc1 == 0 and rc2 == 0 and rc3 == 0
        for i, item in enumerate(items):
            pf, pb, pbb = plain_calls(item, gs[i], gbs[i], rnd)
            assert same(f[i][0], pf[0]) and same(f[i][1], pf[1]) and f[i][2:] == pf[2:], (name, i, rnd)
            assert all_same(b[i], pb) and all_same(bb[i], pbb), (name, i, rnd)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["b_unequal", "b_vec8", "b_y_off"])
def test_a_batch_of_unequal_items_is_its_items(dt, case):
    """relayout.  b_unequal: the linear grid sized by the largest M * hw, the smaller items' waves leaving in front of the wave
    reduction - and, for bfloat16, 8 per lane given up for 4 because ONE hw (256) does not fill 8.  b_vec8: the linear grid at 8 per
    lane, unequal items.  b_y_off: one latent 4 bytes off pulls its aligned neighbour down to 1 per lane."""
    shapes = {"b_unequal": [(2, 16, 16), (5, 16, 16), (1, 16, 32)], "b_vec8": [(2, 16, 32), (3, 32, 32)], "b_y_off": [(2, 16, 16), (2, 16, 16)]}[case]
    items, gs = map(list, zip(*(one(5200 + 10 * len(case) + i, *shp, dt) for i, shp in enumerate(shapes))))
    if case == "b_y_off":
        items[1] = (off(items[1][0]),) + items[1][1:]
    check_batch(case, dt, items, gs)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_one_misaligned_output_takes_the_call_to_one_position_per_lane(dt):
    """relayout: everything aligned except like_out, v_out, g_like, dy or dscales - an address only the C ABI can pass"""
    item, g = one(5300, 2, 16, 16, dt)
    for rnd in (True, False):
        pf, pb, _ = plain_calls(item, g, 1.5, rnd)
        for which in range(2):
            outs = [torch.empty_like(item[0]) for _ in range(2)]
            outs[which] = off(outs[which])
            assert_form("b_out_off", dt, [fitem(*item, rest=outs)], False)
            rc, [f] = raw_forward([item], rnd, outs=[tuple(outs)])
            assert rc == 0 and same(f[0], pf[0]) and same(f[1], pf[1]) and f[2:] == pf[2:], (which, rnd)
        for which in ("g_like", "dy", "dscales"):
            gg = off(g) if which == "g_like" else g
            outs = [torch.empty_like(item[0])] + [torch.empty(item[1].shape, dtype=torch.float32, device=DEV) for _ in range(3)]
            if which != "g_like":
                i = R.GRADS.index(which)
                outs[i] = off(outs[i])
            assert_form("b_out_off", dt, [fitem(*item, rest=[gg] + outs)], True)
            rc, [o] = raw_backward([item], [gg], rnd, outs=[outs])
            assert rc == 0 and all_same(o, pb), (which, rnd)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["b_M0", "b_hw0"])
def test_an_empty_item_beside_a_real_one(dt, case):
    """relayout: M = 0 or hw = 0 with valid pointers -> OK, nothing counted, nothing written for it, the neighbour unchanged"""
    (empty, g0), (real, g1) = one(5400, 2, 16, 16, dt), one(5401, 2, 16, 16, dt)
    sizes = [(0, 256) if case == "b_M0" else (2, 0), (2, 256)]
    for back in (False, True):
        assert_form(case, dt, [fitem(*empty, size=sizes[0]), fitem(*real)], back)
    for rnd in (True, False):
        pf, pb, pbb = plain_calls(real, g1, GB[1], rnd)
        rc, f = raw_forward([empty, real], rnd, fill=-7.0, sizes=sizes)
        assert rc == 0 and f[0][2:] == (0, 0) and torch.all(f[0][0] == -7.0) and torch.all(f[0][1] == -7.0)
        assert same(f[1][0], pf[0]) and same(f[1][1], pf[1]) and f[1][2:] == pf[2:]
        for gs, gb, want in (([g0, g1], None, pb), (None, list(GB[:2]), pbb)):
            outs = [[torch.full_like(it[0], -7.0)] + [torch.full(it[1].shape, -7.0, dtype=torch.float32, device=DEV) for _ in range(3)] for it in (empty, real)]
            torch.cuda.current_stream().synchronize()
            rc, o = raw_backward([empty, real], gs, rnd, g_bits=gb, outs=outs, sizes=sizes)
            assert rc == 0 and all(torch.all(t == -7.0) for t in o[0]) and all_same(o[1], want), (rnd, gb)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_the_pure_rate_call_gives_the_mapped_call_s_bits(dt):
    item, _ = one(5500, 2, 16, 16, dt)
    assert_form("b_rate_only", dt, [fitem(*item, rest=(None, None))], False)
    for rnd in (True, False):
        (rc1, [f]), (rc2, [r]) = raw_forward([item], rnd), raw_forward([item], rnd, outs=[(None, None)])
        assert rc1 == 0 and rc2 == 0 and r[2:] == f[2:] and f[2] > 0 and f[3] == 0


# ---- c. strided planes through the public calls -----------------------------------------------------------------------------------------
def relaid(how, planes):
    """three dense [2, 4M, h, w] planes -> the same values as views that share one set of strides"""
    N, KM, h, w = planes[0].shape
    if how == "chunk":  # what a parameter network's output gives: weights already softmaxed, written into the third chunk
        views = list(planes[0].new_empty((N, 3 * KM, h, w)).chunk(3, 1))
    elif how == "every2":
        views = [p.new_empty((N, 2 * KM, h, w))[:, ::2] for p in planes]
    else:
        views = [p.new_empty((2 * N, KM, h, w))[1::2] for p in planes]
    for v, p in zip(views, planes):
        v.copy_(p)
    return views


def grads_through_rate(gmc, y, s, m, w, gb, training):
    leaves = [t.detach().requires_grad_(True) for t in (y, s, m, w)]
    torch.manual_seed(9)
    outputs, bits = gmc.rate_bits(*leaves, training=training)
    (bits * torch.tensor(gb, dtype=torch.float64, device=DEV)).sum().backward()
    return outputs.detach(), bits.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hw", ["hw64", "hw35"])
@pytest.mark.parametrize("how", ["chunk", "every2", "batch2"])
def test_strided_planes_equal_their_dense_copies(gmc, dt, hw, how):
    """relayout: stride_k, stride_c and the item step other than the dense ones reach both kernels (no copy is made on the way: checked),
    while the gradient planes are written densely"""
    M, (h, w) = 3, {"hw64": (8, 8), "hw35": (5, 7)}[hw]
    y, *dense, g = make(5600 + h, 2, M, h, w, dtype=DT[dt])
    views = relaid(how, dense)
    assert not any(v.is_contiguous() for v in views) and all(torch.equal(v, d) for v, d in zip(views, dense))
    view = gmc._stacked_view(y, *views)
    assert [t.data_ptr() for t in view[:4]] == [t.data_ptr() for t in (y, *views)] and all(a.stride() == b.stride() for a, b in zip(view[1:4], views))
    s_item, sc, es = view[8], view[9], views[0].element_size()
    assert (s_item, sc) != (4 * M * h * w, h * w) and (s_item, sc) == {"chunk": (12 * M * h * w, h * w), "every2": (8 * M * h * w, 2 * h * w), "batch2": (8 * M * h * w, h * w)}[how]
    name = f"c_{how}_{hw}"
    for back in (False, True):
        assert_form(name, dt, [R.form_item(h * w, sc, M * sc, [v.data_ptr() + i * s_item * es for v in views], [y.data_ptr() + i * M * h * w * 4, 0]) for i in range(2)], back)
    for rnd in (True, False):
        v1, like1, grads1 = grads_through_map(gmc, y, *views, g, rnd)
        v2, like2, grads2 = grads_through_map(gmc, y, *dense, g, rnd)
        assert same(v1, v2) and same(like1, like2) and all_same(grads1, grads2), (how, rnd)
        for t, a in zip((y, *views), grads1):
            assert a is None or (a.is_contiguous() and a.shape == t.shape and a.dtype == t.dtype)
    for training in (False, True):
        o1, b1, grads1 = grads_through_rate(gmc, y, *views, list(GB[:2]), training)
        o2, b2, grads2 = grads_through_rate(gmc, y, *dense, list(GB[:2]), training)
        assert same(o1, o2) and torch.equal(b1, b2) and all_same(grads1, grads2) and (grads1[0] is None) == (not training), (how, training)
        assert all(a.is_contiguous() and a.shape == t.shape and a.dtype == t.dtype for t, a in zip(views, grads1[1:]))


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("hw", ["hw64", "hw35"])
def test_strided_planes_through_ctypes_write_only_their_dense_outputs(dt, hw):
    """relayout, with a guard: planes of channel stride 2 * hw are read strided while every output is written at k * M * hw + c * hw.
    Each output is the head of a buffer twice its size, and the tail stays as it was: an output indexed by the inputs' strides would
    land there."""
    M, (h, w) = 3, {"hw64": (8, 8), "hw35": (5, 7)}[hw]
    dense, g = one(5650 + h, M, h, w, dt)
    item = (dense[0], *(p.new_empty((8 * M, h, w))[::2].copy_(p) for p in dense[1:]))
    n, size = M * h * w, (M, h * w, 2 * M * h * w, 2 * h * w)
    for back in (False, True):
        ptrs = [item[0].data_ptr()] + ([g.data_ptr()] if back else [])
        assert_form(f"c_ctypes_{hw}", dt, [R.form_item(h * w, size[3], size[2], [t.data_ptr() for t in item[1:]], ptrs)], back)

    def guarded(counts):
        bufs = [torch.full((2 * c,), -7.0, dtype=torch.float32, device=DEV) for c in counts]
        return bufs, [b[:c].view(-1, h, w) for b, c in zip(bufs, counts)]

    for rnd in (True, False):
        pf, pb, pbb = plain_calls(dense, g, GB[0], rnd)
        bufs, heads = guarded([n, n])
        torch.cuda.current_stream().synchronize()
        rc, [f] = raw_forward([item], rnd, outs=[tuple(heads)], sizes=[size])
        assert rc == 0 and same(f[0], pf[0]) and same(f[1], pf[1]) and f[2:] == pf[2:] and all(torch.all(b[n:] == -7.0) for b in bufs), rnd
        for gs, gb, want in (([g], None, pb), (None, [GB[0]], pbb)):
            bufs, heads = guarded([n, 4 * n, 4 * n, 4 * n])
            torch.cuda.current_stream().synchronize()
            rc, [o] = raw_backward([item], gs, rnd, g_bits=gb, outs=[heads], sizes=[size])
            assert rc == 0 and all_same(o, want), (rnd, gb)
            assert all(torch.all(b[b.numel() // 2:] == -7.0) for b in bufs), (rnd, gb)


# ---- d. partial gradients -------------------------------------------------------------------------------------------------------------------
def test_partial_gradients_through_autograd(gmc):
    """relayout: needs_input_grad subsets make some of dy, dscales, dmeans, dweights NULL; what is asked for equals the all-outputs call"""
    t = make(5700, 2, 2, 16, 16)
    for rnd in (False, True):
        _, like_all, full = grads_through_map(gmc, *t, rnd)
        for subset in [(0,), (1,), (2,), (3,), (1, 3)]:
            leaves = [x.detach().requires_grad_(i in subset) for i, x in enumerate(t[:4])]
            _, like = gmc.likelihood(*leaves, round=rnd)
            like.backward(t[4])
            assert same(like.detach(), like_all)
            for i, leaf in enumerate(leaves):
                assert same(leaf.grad, full[i] if i in subset else None), (rnd, subset, i)


@pytest.mark.parametrize("case", ["d_hw256", "d_hw35"])
def test_every_subset_of_the_four_outputs_through_ctypes(case):
    """relayout, at 4 positions per lane on the linear grid and at 1 on the tiled one"""
    item, g = one(5800, 2, *{"d_hw256": (16, 16), "d_hw35": (5, 7)}[case], "f32")
    assert_form(case, "f32", [fitem(*item, rest=(g,))], True)
    for gs, gb in (([g], None), (None, [GB[0]])):
        rc, [full] = raw_backward([item], gs, False, g_bits=gb)
        assert rc == 0
        for subset in itertools.chain.from_iterable(itertools.combinations(range(4), n) for n in range(1, 5)):
            outs = [torch.full_like(full[i], -7.0) if i in subset else None for i in range(4)]
            rc, [o] = raw_backward([item], gs, False, g_bits=gb, outs=[outs])
            assert rc == 0 and all(same(o[i], full[i]) for i in subset), (subset, gb)


# ---- e. the bounds ------------------------------------------------------------------------------------------------------------------------
def corpus_at(sb, arrays=None):
    cpu = [torch.from_numpy(a) for a in (arrays if arrays is not None else R.corpus(sb=sb))[:5]]
    return cpu, [t.to(DEV) for t in cpu]


@pytest.mark.parametrize("sb,lb", R.BOUNDS)
def test_likelihood_and_gradients_at_other_bounds(sb, lb):
    """accuracy, per region, against R.forward / R.reference_gradients at the same bounds; region (b) is rebuilt around sb.  The floor of
    a likelihood's error is the bound, as in tests/test_gpu_likelihood.py; with lb = 0 it is 2^-126, the smallest normal binary32 -
    below it a binary32 likelihood carries no relative accuracy at all.  The rows whose float64 L is within 1e-3 of lb are left out
    (tests/test_likelihood_cpu.py: under 1 % at each setting).  Then the decisions that only these bounds reach."""
    cpu, gpu = corpus_at(sb)
    gmc = GaussianMixtureConditional(K=4, scale_bound=sb, likelihood_bound=lb).eval()
    lb32 = np.float32(lb)
    floor = float(lb32) if lb > 0 else 2.0 ** -126
    for rnd in (False, True):
        f64, f32 = R.forward(*cpu[:4], rnd=rnd, sb=sb, lb=lb, dtype=torch.float64), R.forward(*gpu[:4], rnd=rnd, sb=sb, lb=lb)
        keep = ~R.near_bound(f64["L"].numpy(), lb)
        assert keep.mean() >= 0.99
        v, like, grads = grads_through_map(gmc, *gpu, rnd)
        like = like.cpu().numpy()
        b64, b32 = R.reference_gradients(*cpu, rnd=rnd, sb=sb, lb=lb)[1], {k: t.cpu().numpy() for k, t in R.backward(f32, gpu[4]).items()}
        for name in R.REGIONS:
            check_accuracy(f"sb {sb:g} lb {lb:g} rnd={int(rnd)} likelihood ({name})", like, f32["out"].cpu().numpy(), f64["out"].numpy(), R.region_mask(name) & keep, floor)
        for gname, got in zip(R.GRADS, grads):
            if got is None:
                continue
            got, want = got.cpu().numpy(), b64[gname].numpy()
            rows = keep if gname == "dy" else np.tile(keep, (1, 4, 1, 1))
            for name in R.REGIONS:
                check_accuracy(f"sb {sb:g} lb {lb:g} rnd={int(rnd)} {gname} ({name})", got, b32[gname], want, (R.region_mask(name) if gname == "dy" else R.plane_mask(name)) & rows)
            assert np.all(got[rows & (want == 0)] == 0), gname  # (the pass-through decisions, as in test_backward_through_the_map_on_the_corpus)
            live = rows & (want != 0)
            assert np.array_equal(got[live] == 0, b32[gname][live] == 0), gname
        L32, g = f32["L"].cpu().numpy(), cpu[4].numpy()
        dw = grads[3].cpu().numpy().reshape(4, *R.SHAPE[1:])
        if lb == 0:
            # no bound: region (c)'s exact zeros and region (g)'s negative L come out as they are, are left out of the rate and counted ...
            assert np.all(like[R.region_mask("c")] == 0) and (like[R.region_mask("g")] < 0).sum() >= 8
            rc, [(lk, _, bits_q, nonfinite)] = raw_forward([tuple(t[0] for t in gpu[:4])], rnd, sb=sb, lb=0.0)
            lk = lk.cpu().numpy().astype(np.float64)
            assert rc == 0 and np.array_equal(lk.astype(np.float32), like[0]) and nonfinite == int((f32["out"] <= 0).sum()) >= 256 + 8
            want_bits = float((-np.log2(lk[lk > 0])).sum())
            print(f"lb 0 rnd={int(rnd)}: bits_q {bits_q} = {bits_q * 2.0 ** -32!r} bits, host float64 sum over the {int((lk > 0).sum())} counted {want_bits!r}")
            assert abs(bits_q * 2.0 ** -32 - want_bits) <= lk.size * 2.0 ** -33 + 1e-12 * abs(want_bits)
            # ... and every gradient passes: below a bound of 1e-9 a positive g at a negative L would be zeroed
            assert b32["pass_like"].all()
            neg = (L32[0] < 0) & (g[0] > 0)
            assert neg.sum() >= 4 and np.all((dw[:, neg] != 0).any(0))
        if lb == 0.5:  # most of region (a) is at the bound: gradients are zero exactly where g >= 0
            below = R.region_mask("a") & keep & (L32 < lb32)
            assert below.mean() > 0.5 * R.region_mask("a").mean() and np.all(like[below] == lb32)
            for gname, got in zip(R.GRADS, grads):
                if got is not None:
                    got = got.cpu().numpy().reshape(-1, *R.SHAPE[1:])
                    assert np.all(got[:, (below & (g >= 0))[0]] == 0), gname
            passed = (below & (g < 0))[0]
            ref_dw = b32["dweights"].reshape(4, *R.SHAPE[1:])  # (zero only where every p_k underflows in binary32: torch's is zero too)
            assert passed.sum() >= 64 and np.array_equal(dw[:, passed] != 0, ref_dw[:, passed] != 0) and (dw[:, passed] != 0).any(0).mean() > 0.8


# ---- f. g_bits on the corpus ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lb", [1e-9, 0.0, 0.5])
@pytest.mark.parametrize("gb", [1.5, -0.375])
def test_g_bits_on_the_corpus_is_the_map_backward_at_its_own_gradient(gb, lb):
    """relayout, by the method of test_backward_through_rate_bits_is_the_map_backward_at_its_own_gradient: the backward at the scalar
    g_bits equals the map backward at R.g_from_bits(out, gb) - 0 for a latent left out of the sum - bit for bit, through rate_bits
    (rounding) and through ctypes (no rounding: dy too).  Then the decisions.  With gb > 0, g < 0 passes below the bound; with gb < 0
    it is zeroed.  In region (c) that shows only as exact zeros either way: every p_k is 0 in binary32 there (|v - mu| >= 45 sigma:
    erfcf underflows; R.forward on the CPU agrees, tests/test_likelihood_cpu.py), so dweights = g * 0.  The decision is therefore
    also asserted where it can be seen: at lb = 0.5, on region (a)'s latents below the bound, dweights is non-zero for gb > 0."""
    cpu, gpu = corpus_at(R.SB)
    gmc = GaussianMixtureConditional(K=4, likelihood_bound=lb).eval()
    _, _, grads = grads_through_rate(gmc, *gpu[:4], [gb], False)
    leaves = [t.detach().requires_grad_(True) for t in gpu[:4]]
    _, like = gmc.likelihood(*leaves, round=True)
    like.backward(R.g_from_bits(like.detach(), gb))
    assert grads[0] is None and leaves[0].grad is None and all(same(a, b.grad) for a, b in zip(grads[1:], leaves[1:]))
    item = [tuple(t[0] for t in gpu[:4])]
    (rc1, [o]), (rc2, [(out, _, _, nonfinite)]) = raw_backward(item, None, False, g_bits=[gb], lb=lb), raw_forward(item, False, lb=lb)
    rc3, [o2] = raw_backward(item, [R.g_from_bits(out, gb)], False, lb=lb)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0 and all_same(o, o2)
    o = [t.cpu().numpy().reshape(-1, *R.SHAPE[1:]) for t in o]
    out = out.cpu().numpy()
    c, a = R.region_mask("c")[0], R.region_mask("a")[0]
    if lb == 0:
        left = ~R.counts(torch.from_numpy(out)).numpy()
        assert nonfinite == left.sum() >= 256 + 8 and (left & (out < 0)).sum() >= 8 and all(np.all(t[:, left] == 0) for t in o)
        assert all((t[:, ~left] != 0).any() for t in o)
    else:
        assert nonfinite == 0 and np.all(out[c] == np.float32(lb)) and all(np.all(t[:, c] == 0) for t in o)
    if lb == 0.5:
        below = a & (out == np.float32(lb))
        assert below.sum() >= 128
        if gb > 0:
            assert np.all((o[3][:, below] != 0).any(0))
        else:
            assert all(np.all(t[:, below] == 0) for t in o)


# ---- g. non-finite inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_non_finite_inputs(dt):
    """relayout away from the planted latents (every output equals the unplanted run's), classes at them (the float32 restatement's, on
    the GPU, from the widened values), n_nonfinite the restatement's count.  Where section 3g's select (`rule ? G : 0`) and the
    reference's `mask * G` part - a NaN or +inf G_k that its rule does not pass - the header is pinned: exact zeros."""
    arrays = R.edge_inputs()
    planted = arrays[5]
    hole = torch.from_numpy(R.planted_mask(planted)[0]).to(DEV)
    hole4 = hole.repeat(4, 1, 1)

    def device(arrs):
        y, s, m, w, g = (dv(a)[0] for a in arrs[:5])
        return (y, *(t.to(DT[dt]) for t in (s, m, w))), g

    (item, g), (plain, _) = device(arrays), device(R.corpus())
    wide = [t.to(torch.float32).unsqueeze(0) for t in item]
    for rnd in (True, False):
        f32 = R.forward(*wide, rnd=rnd)
        (rc1, [f]), (rc2, [pf]) = raw_forward([item], rnd), raw_forward([plain], rnd)
        assert rc1 == 0 and rc2 == 0 and pf[3] == 0
        for got, ref, want in ((f[0], pf[0], f32["out"]), (f[1], pf[1], f32["v"])):
            assert same(got[~hole], ref[~hole]) and np.array_equal(R.classes(got[hole]), R.classes(want[0][hole])), rnd
        left = ~R.counts(f32["out"])
        assert f[3] == int(left.sum()) >= 16 and {0, 1, 4} >= set(R.classes(f[0][hole]).tolist()) >= {0, 4}
        # the sum over the others: the unplanted run's, less its terms at the planted latents, plus theirs where they still count - each
        # term the host's log2 may round one unit apart from the device's
        term = lambda x: np.rint(-np.log2(x.cpu().numpy().astype(np.float64)) * 2.0 ** 32).astype(np.int64).sum()  # noqa: E731
        assert abs(f[2] - (pf[2] - term(pf[0][hole]) + term(f[0][hole & ~left[0]]))) <= 2 * int(hole.sum())
        if rnd:  # ... and through the public call
            _, bits, nf = GaussianMixtureConditional(K=4).eval().rate_bits(*(t.unsqueeze(0) for t in item), return_nonfinite=True)
            assert nf.tolist() == [f[3]] and float(bits[0]) == f[2] * 2.0 ** -32
        for gs, gb, g_ref in (([g], None, g.unsqueeze(0)), (None, [GB[0]], R.g_from_bits(f32["out"], GB[0]))):
            (rc1, [o]), (rc2, [po]) = raw_backward([item], gs, rnd, g_bits=gb), raw_backward([plain], gs, rnd, g_bits=gb)
            assert rc1 == 0 and rc2 == 0
            b32 = R.backward(f32, g_ref)
            for name, got, ref in zip(R.GRADS, o, po):
                h = hole if name == "dy" else hole4
                assert same(got[~h], ref[~h]), (name, rnd, gb)
                assert np.array_equal(R.classes(got[h]), R.classes(b32[name][0][h])), (name, rnd, gb)
            dropped = (~b32["pass_scale"] & ~torch.isfinite(b32["G"]))[0]
            assert int(dropped.sum()) >= 8 and not bool((dropped & ~hole4).any()) and torch.all(o[1][dropped] == 0)
