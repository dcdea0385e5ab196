"""GPU (-m gpu): the kernels AROUND the coder held to the oracle at their edges - ``quant_stats_kernel`` and ``chan_compact_kernel`` in
front of every encode and pricing call, ``yhat_scatter_kernel<int16 / int32>``, ``yhat_scatter_round_kernel`` and
``yhat_zero_dead_kernel`` behind every decode call (flashgmm_amd/csrc/fgmm_kernels.hip) - on the corpus of tests/census_ref.py, built by
placing values: every plane size at which the census changes its path or its trip count, one value on every position where a fold can
lose it, the rounding and sign cases, and channel lists with their edges at 64, 256 and 512.

Everything is exact: abs_max, the zero bitmap, y_q and y_hat as bit patterns, the bytes against ``oracle.encode_gmm``.  The census
kernel picks its float4 or scalar path inside itself; every encode case restates that choice from hw and the addresses it really hands
over (``census_ref.stats_path``) and asserts it is the planned one.  The decode side writes into buffers filled with a NaN pattern, with
guard elements on both sides: a position no kernel writes, and a write outside the latent, both show.  What the corpus must be for
this to mean anything: tests/test_census_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, _boundary, _lib
from flashgmm_amd.entropy_models import _ctx_stream
from tests import census_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POISON = 0x7FC0DEAD  # a NaN no kernel here produces
GUARD = 8


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def ctx_options():
    """set options of the process-wide context for one test and restore them afterwards (gpu_decode back to 0)"""
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


@functools.lru_cache(maxsize=None)
def gmc_of(clamp=True, stride=0):
    return GaussianMixtureConditional(K=4, mode=R.MODE, clamp_scales=clamp, checkpoint_stride=stride)


@functools.lru_cache(maxsize=None)
def expected(oracle, item, kind, clamp):
    """the reference side of an item, once: ``census_ref.Item.expect`` and the oracle's bytes"""
    e = item.expect(kind, clamp)
    e["bytes"] = oracle.encode_gmm(R.MODE, e["sym"], *e["rows"])
    return e


def one_in(t):
    """the same values as a dense view one element into a storage of its own (the element before it: NaN)"""
    buf = torch.full((t.numel() + 1,), float("nan"), dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    v = buf[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4
    return v


class Guarded:
    """n floats on the device between guard elements, everything pre-filled with POISON; ``lead`` = GUARD: 16-byte aligned,
    GUARD + 1: one element in"""

    def __init__(self, n, lead=GUARD):
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + GUARD,), POISON, dtype=torch.int32, device=DEV)
        self.ptr = self.buf.data_ptr() + 4 * lead
        assert self.ptr % 16 == 4 * (lead - GUARD)

    def read(self, name):
        a = self.buf.cpu().numpy()
        assert np.all(a[:self.lead] == POISON) and np.all(a[self.lead + self.n:] == POISON), f"{name}: a guard element was written"
        return a[self.lead:self.lead + self.n].view(np.float32)


def planes_of(item, kind="float32"):
    return [dv(a) for a in item.device_planes(kind)[0]]


def check_encoded(oracle, item, kind, clamp, got, yq, name):
    """one item's ((bytes, abs_max, zero_bitmap), y_q) against the reference side; a failure of the bytes names the first channel of
    the expected compact list whose symbols differ"""
    e = expected(oracle, item, kind, clamp)
    b, am, zb = got
    assert (am, [int(v) for v in zb]) == (e["am"], e["zb"].tolist()), (name, am, e["am"])
    assert R.same_bits(yq.reshape(-1), e["yq"].reshape(-1)), (name, np.nonzero(R.bits(yq.reshape(-1)) != R.bits(e["yq"].reshape(-1)))[0][:8])
    if bytes(b) != e["bytes"]:
        raise AssertionError(f"{name}: bytes differ; first channel of the compact list with other symbols: {R.first_wrong_channel(oracle, bytes(b), e, item.hw)}")
    if isinstance(b, CheckpointedBytes):
        assert b.ckpt_stride == R.STRIDE and len(b.ckpt) == max(len(e["sym"]) - 1, 0) // R.STRIDE, name


def compress_list(oracle, items, kind="float32", clamp=True, stride=0, want_path=None):
    """ONE compress_batch call of the sequence form on ``items``, every tensor an allocation of its own, checked item by item
    -> the call's results"""
    ys = [dv(it.y) for it in items]
    ps = [planes_of(it, kind) for it in items]
    if want_path is not None:  # (y_q is the library's allocation: taken as aligned before the call, read off it after)
        assert [R.stats_path(it.hw, y.data_ptr()) for it, y in zip(items, ys)] == want_path
    res = gmc_of(clamp, stride).compress_batch(ys, *([p[k] for p in ps] for k in range(3)))
    for it, y, ((b, am, zb), yq) in zip(items, ys, res):
        if want_path is not None:
            assert R.stats_path(it.hw, y.data_ptr(), yq.data_ptr()) == want_path[0]
        check_encoded(oracle, it, kind, clamp, (b, am, zb.tolist()), yq.cpu().numpy(), f"{it.name} {kind} clamp={clamp} stride={stride}")
    return res, ps


# ---- a. the encode side -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("placement", R.PLACEMENTS)
def test_sizes_under_every_placement(oracle, placement, clamp):
    """hw = 1 .. 2052 - less than a wave, one lane into the next wave / block / trip, one and two trips of the float4 path - with y
    and the y_q output aligned, one element in, and as views of a batch: the path the kernel takes is asserted before the call"""
    gmc = gmc_of(clamp)
    for hw in R.SIZES:
        want = R.planned_paths(hw, placement)
        name = f"hw={hw} {placement} clamp={clamp}"
        if placement == "batch_view":
            items = [R.size_item(hw), R.size_item(hw, True)]
            big = torch.full((3, R.SIZE_M, 1, hw), float("nan"), device=DEV)
            big[0], big[2] = dv(items[0].y)[0], dv(items[1].y)[0]
            view = big[::2]
            ys = [view[0:1], view[1:2]]
            assert [y.data_ptr() - big.data_ptr() for y in ys] == [a for a, _ in R.planned_addresses(hw, placement)]
            ps = [planes_of(it) for it in items]
            assert [R.stats_path(hw, y.data_ptr()) for y in ys] == want, name
            res = gmc.compress_batch(ys, *([p[k] for p in ps] for k in range(3)))
            for it, y, ((b, am, zb), yq) in zip(items, ys, res):
                assert R.stats_path(hw, y.data_ptr(), yq.data_ptr()) in want
                check_encoded(oracle, it, "float32", clamp, (b, am, zb.tolist()), yq.cpu().numpy(), name)
            assert torch.isnan(big[1]).all()
            continue
        item = R.size_item(hw)
        y = dv(item.y)
        if placement == "y_off":
            y = one_in(y)
        if placement != "yq_off":
            assert [R.stats_path(hw, y.data_ptr())] == want, name
            (got, yq), = gmc.compress_batch([y], *([p] for p in planes_of(item)))
            assert [R.stats_path(hw, y.data_ptr(), yq.data_ptr())] == want, name
            check_encoded(oracle, item, "float32", clamp, (got[0], got[1], got[2].tolist()), yq.cpu().numpy(), name)
            continue
        # the y_q output one element in: through the C ABI, into a guarded buffer
        out, keep = Guarded(item.M * hw, GUARD + 1), []
        yp, sp, mp, wp, M, hw_, sk, sc, dev, dt = gmc._item_ints(y, *planes_of(item), keep)
        zb = torch.empty(M, dtype=torch.int64)
        assert (yp % 16, out.ptr % 16) == (0, 4) and [R.stats_path(hw, yp, out.ptr)] == want == ["scalar"], name
        strings, ams = _boundary.compress_items(*_ctx_stream(dev), [(yp, sp, mp, wp, M, hw_, sk, sc, out.ptr, zb.data_ptr(), dt)], 0, gmc._mode(),
                                                int(clamp), 0)
        check_encoded(oracle, item, "float32", clamp, (strings[0], ams[0], zb.tolist()), out.read(name), name)


@pytest.mark.parametrize("variant", [("float32", True, 0), ("float32", False, 0), ("float16", True, 0), ("float32", True, R.STRIDE)],
                         ids=["f32", "f32-noclamp", "f16", "f32-ckpt"])
@pytest.mark.parametrize("hw", R.SWEEP_HW)
def test_position_sweep(oracle, hw, variant):
    """one value - the channel's only non-zero, its negative extreme, a NaN, +inf - on each position where a fold can lose it: the
    fourth float4 component, wave 0's last lane, wave 3's first, the end of a partial trip.  The items with one channel per position
    show it in the zero bitmap, y_q and the bytes; the one-channel items (one batched call per kind) in abs_max"""
    kind, clamp, stride = variant
    path = R.stats_path(hw, 0)
    for k in R.KINDS:
        compress_list(oracle, [R.sweep_item(hw, k)], kind, clamp, stride, want_path=[path])
    for k in R.SOLO_KINDS:
        items = R.sweep_solos(hw, k)
        res, _ = compress_list(oracle, items, kind, clamp, stride, want_path=[path] * len(items))
        assert [r[0][1] for r in res] == [R.SOLO_ABS_MAX[k]] * len(items)


@pytest.mark.parametrize("clamp", [True, False])
def test_rounding_and_sign(oracle, clamp):
    """nz is taken on the ROUNDED value (+-0.5, -0.3 -> -0.0 and denormals leave a channel dead; 0.50000006, 1.5 and 2.5 -> 2 do not),
    abs_max on the unrounded extremes, truncated; y_q bit for bit"""
    for hw in R.ROUND_HW:
        items = [R.rounding_item(name, hw) for name, *_ in R.ROUNDING]
        res, _ = compress_list(oracle, items, clamp=clamp, want_path=[R.stats_path(hw, 0)] * len(items))
        for (name, _, live, am), ((_, am_g, zb), _) in zip(R.ROUNDING, res):
            assert (am_g, zb.tolist()) == (am, [int(live)] * 2), (name, hw)


@pytest.mark.parametrize("variant", [("float32", True, 0), ("float32", False, 0), ("float16", True, 0), ("float32", True, R.STRIDE)],
                         ids=["f32", "f32-noclamp", "f16", "f32-ckpt"])
@pytest.mark.parametrize("M", R.COMPACT_M)
def test_channel_compaction(oracle, M, variant):
    """chan_list and its count through the bytes: live channels on both sides of 63 | 64, 255 | 256 and 511 | 512, a chunk of 256 and
    a wave without a live channel in front of live ones, no live channel at all - each item a call of its own"""
    kind, clamp, stride = variant
    for name in R.live_sets(M):
        compress_list(oracle, [R.compact_item(M, name)], kind, clamp, stride)


def pricing_items():
    items = [R.size_item(hw) for hw in R.SIZES]
    for hw in R.SWEEP_HW:
        items += [R.sweep_item(hw, k) for k in R.KINDS]
        for k in R.SOLO_KINDS:
            items += R.sweep_solos(hw, k)
    items += [R.rounding_item(name, hw) for name, *_ in R.ROUNDING for hw in R.ROUND_HW]
    return items + [R.compact_item(M, name) for M, name in R.COMPACT_CASES]


@pytest.mark.parametrize("family", ["size", "sweep", "solo", "rounding", "compact"])
def test_pricing_calls_share_the_census(oracle, family):
    """estimate_bits_batch and quantize_rdo_batch at lambda = 0 run the same front half: n_symbols, abs_max and the zero bitmap of the
    estimate are the coder's; the RDOQ call returns round(y) (+0.0 for zero) and the census OF THAT - the zero bitmap is the coder's,
    abs_max the one compressing round(y) returns (include/flashgmm_amd.h section 3c)"""
    items = [it for it in pricing_items() if it.name.startswith(family)]
    assert len(items) >= 8
    gmc = gmc_of()
    ys, ps = [dv(it.y) for it in items], [planes_of(it) for it in items]
    args = (ys, *([p[k] for p in ps] for k in range(3)))
    est = gmc.estimate_bits_batch(*args)
    rdo = gmc.quantize_rdo_batch(*args, 0.0)
    for it, r, q in zip(items, est, rdo):
        e = expected(oracle, it, "float32", True)
        assert (r.n_symbols, r.abs_max, r.zero_bitmap.tolist()) == (len(e["sym"]), e["am"], e["zb"].tolist()), it.name
        rounded = R.Item("rounded", e["yq"] + np.float32(0.0), it.planes)  # (-0.0 + 0.0 = +0.0)
        assert R.same_bits(q.y.cpu().numpy(), rounded.y), it.name
        assert (q.n_changed, q.abs_max, q.zero_bitmap.tolist()) == (0, rounded.expect()["am"], e["zb"].tolist()), it.name


# ---- b. the decode side, on a poisoned output ------------------------------------------------------------------------------------------
def decode_poisoned(gmc, streams, abs_maxes, items, planes):
    """fgmm_gmc_decompress_batch through the C ABI, every y_hat a guarded buffer full of POISON, every second one one element in
    -> per item the floats found there (the guards checked)"""
    keep, tuples, outs = [], [], []
    for i, (it, p) in enumerate(zip(items, planes)):
        _, sp, mp, wp, M, hw, sk, sc, dev, dt = gmc._item_ints(None, *p, keep)
        out = Guarded(M * hw, GUARD + i % 2)
        zb = torch.from_numpy(it.expect()["zb"].copy())
        keep.append(zb)
        outs.append(out)
        tuples.append((sp, mp, wp, M, hw, sk, sc, out.ptr, zb.data_ptr(), dt))
    _boundary.decompress_items(*_ctx_stream(torch.device(DEV)), list(streams), [int(a) for a in abs_maxes], tuples, 0, gmc._mode(),
                               int(gmc.clamp_scales), CheckpointedBytes)
    return [out.read(it.name) for it, out in zip(items, outs)]


def check_decoded(items, got, what):
    for it, g in zip(items, got):
        want = it.decoded().reshape(-1)
        bad = np.nonzero(R.bits(g) != R.bits(want))[0]
        dead = np.repeat(it.expect()["zb"] == 0, it.hw)
        assert len(bad) == 0, (f"{what}: {it.name}: {len(bad)} elements differ, first at channel {bad[0] // it.hw} position {bad[0] % it.hw} "
                               f"({'dead' if dead[bad[0]] else 'live'} channel; found {g[bad[0]]!r} / {R.bits(g)[bad[0]]:#x}, expected {want[bad[0]]!r})")


DECODE_CONFIGS = [  # (id, the streams carry notes, options)
    ("plain-rounds", False, dict(scatter_rounds=1)),
    ("plain-rounds-4-pieces", False, dict(scatter_rounds=1, pieces=4)),  # (rounds whose bounds fall inside a channel)
    ("plain-whole", False, dict(scatter_rounds=0)),
    ("generic-rounds", False, dict(scatter_rounds=1, tab_cap_e=256)),
    ("generic-whole", False, dict(scatter_rounds=0, tab_cap_e=256)),
    ("ckpt-auto-rounds", True, dict(gpu_decode=0, scatter_rounds=1)),  # (the items too short for a note go by rounds or whole)
    ("ckpt-auto-whole", True, dict(gpu_decode=0, scatter_rounds=0)),
    ("ckpt-segdec-rounds", True, dict(gpu_decode=1, scatter_rounds=1)),
    ("ckpt-segdec-whole", True, dict(gpu_decode=1, scatter_rounds=0)),
]


@pytest.mark.parametrize("config", DECODE_CONFIGS, ids=[c[0] for c in DECODE_CONFIGS])
def test_decode_writes_every_element_and_nothing_else(oracle, ctx_options, config):
    """after a decode call every element of every dead channel is +0.0, every live element the oracle's symbol, and the guards are
    untouched - symbols returned round by round (yhat_scatter_round_kernel + yhat_zero_dead_kernel) or whole (yhat_scatter_kernel), from
    the single-pass tables, the generic ones, the host's segments and the GPU's segment decoder"""
    what, notes, opts = config
    items = R.decode_items()
    gmc = gmc_of(True, R.STRIDE if notes else 0)
    res, planes = compress_list(oracle, items, stride=R.STRIDE if notes else 0)
    streams = [r[0][0] for r in res]
    assert all(isinstance(b, CheckpointedBytes) == notes for b in streams) and (not notes or sum(len(b.ckpt) > 0 for b in streams) >= 10)
    _lib.set_profiling(0, True)  # (the single-pass kernel counts its edges only then)
    try:
        ctx_options(**opts)
        abs_maxes = [r[0][1] for r in res]
        if "tab_cap_e" in opts:  # (a window of at most 16 edges fits the smallest LDS budget: those items are handed a wider one)
            abs_maxes = [max(a, R.GENERIC_ABS_MAX) for a in abs_maxes]
        got = decode_poisoned(gmc, streams, abs_maxes, items, planes)
        if "tab_cap_e" in opts:
            assert _lib.ctx_stat(0, 3) == 0, "the generic kernels did not run"
        elif not notes:
            assert _lib.ctx_stat(0, 3) > 0, "the single-pass kernel did not run"
        if opts.get("gpu_decode") == 1:
            assert _lib.ctx_stat(0, 4) > 0, "the segment decoder took no bitstream"
    finally:
        _lib.set_profiling(0, False)
    check_decoded(items, got, what)


@pytest.mark.parametrize("rounds", [1, 0])
def test_wide_scatter_meets_a_compact_list_that_is_not_the_identity(oracle, ctx_options, rounds):
    """a bypass symbol beyond int16 in an item whose every second channel is dead: the 32-bit yhat_scatter_kernel goes through
    ``rank`` - given the honest half-width (the generic kernels, scattered whole) and given the half-width of the latent without its
    outlier (the rounds read int16 and the item is scattered once more, wide)"""
    item, clean = R.compact_item(*R.OUTLIER_CASE, outlier=True), R.compact_item(*R.OUTLIER_CASE)
    others = [R.compact_item(513, "alternate"), R.compact_item(64, "none")]
    ctx_options(scatter_rounds=rounds)
    res, planes = compress_list(oracle, [item] + others)
    assert res[0][0][1] == 70001
    for am in (70001, clean.expect()["am"]):
        got = decode_poisoned(gmc_of(), [r[0][0] for r in res], [am] + [r[0][1] for r in res[1:]], [item] + others, planes)
        check_decoded([item] + others, got, f"abs_max {am} rounds={rounds}")
        assert float(np.abs(got[0]).max()) == 70000.0


# ---- c. batches of unequal items -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [0, R.STRIDE])
def test_unequal_items_in_one_call(oracle, ctx_options, stride):
    """M = 513 next to M = 1, an all-dead item between two live ones, in ONE compress_batch / decompress_batch call of the sequence
    form: the ``c >= M`` guards and the item index of every kernel here under unequal items.  Each result is its single-item call's"""
    items = [R.compact_item(M, name) for M, name in R.BATCH_CASES]
    gmc = gmc_of(True, stride)
    res, planes = compress_list(oracle, items, stride=stride)
    singles = [compress_list(oracle, [it], stride=stride)[0][0] for it in items]
    for it, ((b, am, zb), yq), ((b1, am1, zb1), yq1) in zip(items, res, singles):
        assert (bytes(b), am, zb.tolist()) == (bytes(b1), am1, zb1.tolist()) and torch.equal(yq, yq1), it.name
        if stride:
            assert np.array_equal(b.ckpt, b1.ckpt), it.name
    args = ([r[0][0] for r in res], [r[0][1] for r in res], [r[0][2] for r in res])
    for opts in (dict(scatter_rounds=1), dict(scatter_rounds=0)) + ((dict(gpu_decode=1),) if stride else ()):
        ctx_options(scatter_rounds=1, gpu_decode=0)
        ctx_options(**opts)
        out = gmc.decompress_batch(*args, *([p[k] for p in planes] for k in range(3)))
        for i, it in enumerate(items):
            want = it.decoded()
            assert R.same_bits(out[i].cpu().numpy(), want), (it.name, opts)
            one = gmc.decompress_batch([args[0][i]], [args[1][i]], [args[2][i]], *([planes[i][k]] for k in range(3)))[0]
            assert torch.equal(out[i].view(torch.int32), one.view(torch.int32)), (it.name, opts)
        check_decoded(items, decode_poisoned(gmc, *args[:2], items, planes), f"batch {opts}")
