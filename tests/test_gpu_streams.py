"""GPU (-m gpu): the caller's-stream contract of include/flashgmm_amd.h section 2 - "`stream` is the hipStream_t the caller's producer
kernels were enqueued on; the library orders its own work after it and returns with all outputs complete" - on real side streams.

Everywhere else in the suite the caller's stream is the legacy default stream and the inputs are complete before the call, so an
operation the library put on another stream, a plain hipMemcpy that read too early, or a call that returned before its last copy
had landed would still give the right answer.  Here every call is made under ``torch.cuda.stream(s)`` while the PRODUCER of its
inputs is still pending on ``s`` (``pending`` below):

  * the device buffers the call is given hold a DECOY - other values of the same shapes, whose result is asserted to differ from the
    true one, so a read that is not ordered after the producer gives a wrong answer, never a vacuous pass;
  * on ``s``: a delay, then the copies that bring the true values; an event recorded behind them must not have completed when the call
    is made (asserted: a producer that had already finished is a failure of the case, not a skip);
  * the result must be the true inputs' - computed beforehand on the default stream, fully synchronised, or by the oracle;
  * immediately after the call returns, with no synchronisation, the outputs are cloned on a third stream that has never waited for
    ``s``; the clones must be right too ("returns with all outputs complete").  This applies to what the library itself writes; what a
    Python codec assembles afterwards with torch operations is ordered on ``s`` as any torch result is, and is compared after ``s``.

The one pair of entry points that does not synchronise, ``ckbd_unembed`` / ``ckbd_embed``, is stream-ordered (header, section 5): its
results are checked on the same stream and on another stream behind an event.

The delay is ``torch.cuda._sleep``, calibrated with events when the module starts to DELAY_MS = 8 ms.  Measured on an MI355X:
  * the delay: ``_sleep(1_000_000)`` takes 0.433 ms, the calibrated delay 7.70 ms (five runs: 7.696 .. 7.700 ms, by events);
  * the host time between ``ev.record()`` and the entry of the first native call: 15 .. 67 us once a kind of call has been made
    (compress 15 .. 38, decompress 25 .. 50, quantize_rdo 22 .. 67, estimate_bits 15 .. 27), 100 .. 185 us for the first call of a kind.
So the producer outlasts the gap by more than 100 times for every warm call (8 ms = 100 * 80 us) and by more than 40 times for the
slowest first call; the event query is the proof in each single case.  The module takes about 4 s.
"""
import contextlib
import threading
import time
import types

import numpy as np
import pytest
import torch

from flashgmm_amd import GaussianMixtureConditional, ParameterHead, _lib
from helpers import expand_trimmed, hdr_form
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = ["polya", "as", "logistic"]
DEV = "cuda:0"
DELAY_MS = 8.0
LAMBDAS = [0.0, 0.1, 0.5, 2.0]


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def streams():
    """(s1, s2, third): two caller's streams, and the stream that never waits for either"""
    return torch.cuda.Stream(DEV), torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)


@pytest.fixture(scope="module")
def delay():
    """-> delay(times=1): about times * DELAY_MS of GPU time on the current stream (torch.cuda._sleep, its unit measured here with
    events)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 1_000_000
    torch.cuda._sleep(probe)  # (the first launch loads the kernel)
    torch.cuda.synchronize()
    a.record()
    torch.cuda._sleep(probe)
    b.record()
    b.synchronize()
    cycles = int(probe * DELAY_MS / max(a.elapsed_time(b), 1e-3))
    a.record()
    torch.cuda._sleep(cycles)
    b.record()
    b.synchronize()
    assert a.elapsed_time(b) >= 0.5 * DELAY_MS, (cycles, a.elapsed_time(b))
    return lambda times=1: torch.cuda._sleep(times * cycles)


@contextlib.contextmanager
def pending(s, delay, true, decoy, times=1):
    """THE helper.  ``true`` / ``decoy``: device tensors of the same shapes.  Inside the block ``s`` is the current stream and the
    yielded buffers - which hold the decoy - are being overwritten with the true values by copies queued on ``s`` behind a delay
    that has not run out: the call made first thing in the block has a pending producer.  On leaving, ``s`` is synchronised.
    (Only streams are waited for here, never the device: a device-wide wait in one thread holds up the runtime calls of the other
    threads until every stream is idle - their producers included, which would then have finished before their calls were made.)"""
    torch.cuda.current_stream().synchronize()  # (true and decoy were made on the default stream)
    with torch.cuda.stream(s):
        bufs = [d.clone() for d in decoy]
        s.synchronize()
        t0 = time.perf_counter()
        delay(times)
        for b, t in zip(bufs, true):
            b.copy_(t)
        ev = torch.cuda.Event()
        ev.record()
        assert not ev.query(), f"the producer had completed before the call was made, {1e3 * (time.perf_counter() - t0):.2f} ms after it was queued: the case would prove nothing"
        yield bufs
    s.synchronize()


def snapshot(third, outs):
    """clones of the device tensors ``outs`` made on ``third``, which has never waited for the caller's stream, right after a call
    returned and without any synchronisation in between"""
    with torch.cuda.stream(third):
        clones = [o.clone() for o in outs]
    third.synchronize()
    return clones


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


def oracle_bytes(oracle, mode, y, sg, mu, pi):
    sym, s, m, w, am, zb, yq = T.to_coder_inputs(y, *(np.asarray(a, dtype=np.float32) for a in (sg, mu, pi)))
    return oracle.encode_gmm(mode, sym, s, m, w), am, zb, yq


# ---- a. compress -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_compress_with_a_pending_producer(oracle, streams, delay, mode):
    s1, s2, third = streams
    gmc = GaussianMixtureConditional(K=4, mode=mode)
    lat = [T.make_latent(9100 + i, 16, 16, 16) for i in range(6)]
    want = [oracle_bytes(oracle, mode, *l) for l in lat]
    assert len({w[0] for w in want}) == 6  # every decoy's bitstream differs from the true one
    true, decoy = [[dv(a) for a in l] for l in lat[:3]], [[dv(a) for a in l] for l in lat[3:]]

    # one item
    with pending(s1, delay, true[0], decoy[0]) as t:
        (b, am, zb), yq = gmc.compress(*t)
        (yq_3,) = snapshot(third, [yq])
    assert b == want[0][0] and am == want[0][1] and zb.tolist() == want[0][2].tolist()
    assert np.array_equal(yq.cpu().numpy(), want[0][3]) and np.array_equal(yq_3.cpu().numpy(), want[0][3])

    # a list of three, and the same three stacked
    flat = lambda items: [t for it in items for t in it]  # noqa: E731
    with pending(s2, delay, flat(true), flat(decoy)) as t:
        res = gmc.compress_batch(t[0::4], t[1::4], t[2::4], t[3::4])
        yq_3 = snapshot(third, [r[1] for r in res])
    for i in range(3):
        (b, am, zb), yq = res[i]
        assert b == want[i][0] and am == want[i][1] and zb.tolist() == want[i][2].tolist(), i
        assert np.array_equal(yq.cpu().numpy(), want[i][3]) and np.array_equal(yq_3[i].cpu().numpy(), want[i][3]), i
    stack = lambda items: [torch.cat([it[k] for it in items]) for k in range(4)]  # noqa: E731
    with pending(s1, delay, stack(true), stack(decoy)) as t:
        res = gmc.compress_batch(*t)
        yq_3 = snapshot(third, [r[1] for r in res])
    for i in range(3):
        (b, am, zb), yq = res[i]
        assert b == want[i][0] and am == want[i][1] and zb.tolist() == want[i][2].tolist(), i
        assert np.array_equal(yq.cpu().numpy().reshape(want[i][3].shape), want[i][3]), i
        assert np.array_equal(yq_3[i].cpu().numpy().reshape(want[i][3].shape), want[i][3]), i

    # float16 planes: the oracle on the widened values
    l16 = [(l[0],) + tuple(T.to_float16_planes(*l[1:])) for l in (lat[0], lat[3])]
    w16 = [oracle_bytes(oracle, mode, *l) for l in l16]
    assert w16[0][0] != w16[1][0]
    with pending(s2, delay, [dv(a) for a in l16[0]], [dv(a) for a in l16[1]]) as t:
        assert t[1].dtype == torch.float16
        (b, am, zb), yq = gmc.compress(*t)
        (yq_3,) = snapshot(third, [yq])
    assert b == w16[0][0] and am == w16[0][1] and np.array_equal(yq_3.cpu().numpy(), w16[0][3])

    # weights as logits (softmax over K inside the kernel): against the same call on the default stream
    lg = [[dv(l[0]), dv(l[1]), dv(l[2]), dv(np.log(np.maximum(l[3], 1e-6)).astype(np.float32))] for l in (lat[1], lat[4])]
    (b0, am0, zb0), yq0 = gmc.compress(*lg[0], weights_are_logits=True)
    assert bytes(b0) != bytes(gmc.compress(*lg[1], weights_are_logits=True)[0][0])
    with pending(s1, delay, lg[0], lg[1]) as t:
        (b, am, zb), yq = gmc.compress(*t, weights_are_logits=True)
        (yq_3,) = snapshot(third, [yq])
    assert bytes(b) == bytes(b0) and am == am0 and torch.equal(zb, zb0) and torch.equal(yq, yq0) and torch.equal(yq_3, yq0)


# ---- b. decompress -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["table", "host_segments", "gpu_segments"])
def test_decompress_with_pending_parameter_planes(streams, delay, form):
    s1, s2, third = streams
    shape, stride = ((16, 16, 16), 0) if form == "table" else ((40, 16, 12), 256)
    options = {"table": {}, "host_segments": {"gpu_decode": 2, "ckpt_decode": 1}, "gpu_segments": {"gpu_decode": 1}}[form]
    gmc = GaussianMixtureConditional(K=4, mode="polya", checkpoint_stride=stride)
    lat = [T.make_latent(9200 + i, *shape, clamp=False, zero_frac=0.2) for i in range(6)]
    true, decoy = [[dv(a) for a in l] for l in lat[:3]], [[dv(a) for a in l] for l in lat[3:]]
    res = gmc.compress_batch(*([t[k] for t in true] for k in range(4)))
    strings, ams, zbs, want = [r[0][0] for r in res], [r[0][1] for r in res], [r[0][2] for r in res], [r[1] for r in res]
    assert all(torch.equal(w, torch.round(t[0])) for w, t in zip(want, true))
    if stride:
        assert all(len(b.ckpt) > 0 for b in strings)
    saved = {k: _lib.get_option(0, k) for k in options}
    try:
        for k, v in options.items():
            _lib.set_option(0, k, v)
        for i in range(3):  # the decoy's planes decode every stream to something else, or not at all
            try:
                assert not torch.equal(gmc.decompress(strings[i], ams[i], zbs[i], *decoy[i][1:]), want[i]), i
            except RuntimeError:
                pass
        with pending(s1, delay, true[0][1:], decoy[0][1:]) as p:
            y_hat = gmc.decompress(strings[0], ams[0], zbs[0], *p)
            (y_hat_3,) = snapshot(third, [y_hat])
            if form == "gpu_segments":
                assert _lib.ctx_stat(0, 4) == 1  # decoded by the GPU's segment decoder
        assert torch.equal(y_hat, want[0]) and torch.equal(y_hat_3, want[0])
        flat = lambda items: [t for it in items for t in it[1:]]  # noqa: E731
        with pending(s2, delay, flat(true), flat(decoy)) as p:
            outs = gmc.decompress_batch(strings, ams, zbs, p[0::3], p[1::3], p[2::3])
            outs_3 = snapshot(third, outs)
        assert same(outs, want) and same(outs_3, want)
    finally:
        for k, v in saved.items():
            _lib.set_option(0, k, v)


# ---- c. the rate and RDO calls -----------------------------------------------------------------------------------------------------
def key(q):
    return (q.y.cpu().numpy().tobytes(), q.n_changed, q.bits_q_before, q.bits_q_after, q.abs_max, q.zero_bitmap.tolist(),
            None if q.channel_bits_q_after is None else q.channel_bits_q_after.tolist())


def skey(q):
    return key(q) + (q.n_skipped, q.n_eligible, q.ddist_q, None if q.skipped is None else q.skipped.tolist())


def bkey(q):
    return key(q) + (q.lam, q.bytes_pred, q.budget_met, q.passes)


def ckey(c):
    return (c.lambdas, c.bits_q_before, c.bits_q_after, c.n_changed, c.ddist_q, c.n_symbols)


def ekey(e):
    return (e.bits_q, e.nbytes, e.n_symbols, e.n_bypass, e.abs_max, e.zero_bitmap.tolist(), e.channel_bits_q.tolist(),
            e.latent_bits.cpu().numpy().tobytes())


def rate_calls(gmc, budget, cw, pw):
    """name -> (call on four tensors, its key, the device tensors among its outputs)"""
    return {
        "estimate_bits": (lambda t: gmc.estimate_bits(*t, per_channel=True, per_latent=True), ekey, lambda r: [r.latent_bits]),
        "quantize_rdo": (lambda t: gmc.quantize_rdo(*t, 0.5, per_channel=True), key, lambda r: [r.y]),
        "rd_curve": (lambda t: gmc.rd_curve(*t, LAMBDAS), ckey, lambda r: []),
        "quantize_to_budget": (lambda t: gmc.quantize_to_budget(*t, budget), bkey, lambda r: [r.y]),
        "weighted": (lambda t: gmc.quantize_rdo(*t, 0.5, per_channel=True, channel_weights=cw, position_weights=pw), key, lambda r: [r.y]),
        "channel_skip": (lambda t: gmc.quantize_rdo(*t, 0.5, per_channel=True, channel_skip=True), skey, lambda r: [r.y]),
    }


@pytest.mark.parametrize("name", ["estimate_bits", "quantize_rdo", "rd_curve", "quantize_to_budget", "weighted", "channel_skip"])
def test_rate_and_rdo_calls_with_a_pending_producer(streams, delay, name):
    s1, s2, third = streams
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    true, decoy = ([dv(a) for a in T.make_latent(9300 + i, 16, 16, 16, zero_frac=0.2)] for i in range(2))
    ends = gmc.rd_curve(*true, [0.0, 16.0]).nbytes
    assert ends[1] < ends[0]
    cw = torch.linspace(0.25, 4.0, 16, device=DEV)
    pw = (1.0 + (torch.arange(256, device=DEV) % 3).float()).reshape(16, 16)
    call, k, device_outs = rate_calls(gmc, (ends[0] + ends[1]) // 2, cw, pw)[name]
    want_r = call(true)
    want = k(want_r)
    assert want != k(call(decoy))
    if name == "weighted":
        assert want != key(gmc.quantize_rdo(*true, 0.5, per_channel=True))  # (the weights matter)
    with pending(s1 if name in ("estimate_bits", "rd_curve", "weighted") else s2, delay, true, decoy) as t:
        got = call(t)
        outs_3 = snapshot(third, device_outs(got))
    assert k(got) == want and same(outs_3, device_outs(want_r))


# ---- d. the parameter head ---------------------------------------------------------------------------------------------------------
def _fused_codec(M, seed, arithmetic):
    """CheckerboardLatentCodec(fuse_head=...) over real convolutions, as tests/test_gpu_head.py builds it"""
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    torch.manual_seed(seed)
    ctx_net = torch.nn.Conv2d(M, 2 * M, 5, padding=2).to(DEV)
    last = torch.nn.Conv2d(96, 12 * M, 1)
    with torch.no_grad():
        last.bias[: 4 * M] += 1.0  # sigma mostly positive
    ep = torch.nn.Sequential(torch.nn.Conv2d(4 * M, 96, 1), torch.nn.LeakyReLU(), last).to(DEV)
    return CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4, mode="polya")}, entropy_parameters=ep,
                                   context_prediction=ctx_net, fuse_head=True if arithmetic == "f32" else arithmetic)


def codec_key(enc):
    return [(bytes(b), int(am), [int(v) for v in zb.tolist()]) for (b, am, zb) in enc["strings"]], enc["shape"], enc["y_hat"].cpu().numpy().tobytes()


@pytest.mark.parametrize("arithmetic", ["f32", "bf16x6"])
def test_parameter_head_with_pending_weights_and_features(streams, delay, arithmetic):
    s1, s2, third = streams
    M, c_in, h, w = 24, 40, 5, 7
    conv, x, _ = T.make_head(9400, M, c_in, h, w, N=2)
    conv_d, x_d, _ = T.make_head(9401, M, c_in, h, w, N=2)
    wb = lambda c: [c.weight.detach(), c.bias.detach()]  # noqa: E731
    want = torch.cat(ParameterHead(conv, arithmetic=arithmetic).params(x), 1)
    assert not torch.equal(want, torch.cat(ParameterHead(conv_d, arithmetic=arithmetic).params(x), 1))
    assert not torch.equal(want, torch.cat(ParameterHead(conv, arithmetic=arithmetic).params(x_d), 1))
    # the head is created (its weights packed) while the weights are still being written ...
    with pending(s1, delay, wb(conv), wb(conv_d)) as (wt, bias):
        head = ParameterHead(types.SimpleNamespace(weight=wt, bias=bias), arithmetic=arithmetic)
    # ... and used on another stream, with the features pending there
    with pending(s2, delay, [x], [x_d]) as (xb,):
        planes = head.params(xb)
        planes_3 = snapshot(third, planes)
    assert torch.equal(torch.cat(planes, 1), want) and torch.equal(torch.cat(planes_3, 1), want)

    # the codec that owns such a head, compress and decompress whole under a side stream
    Mc, hc, wc = 32, 16, 24
    rng = np.random.default_rng(9402)
    ys = [dv((rng.standard_normal((1, Mc, hc, wc)) * 4).astype(np.float32)) for _ in range(2)]
    sides = [dv(rng.standard_normal((1, 2 * Mc, hc, wc)).astype(np.float32)) for _ in range(2)]
    with torch.no_grad():
        codec = _fused_codec(Mc, 9403, arithmetic)
        want_enc = codec.compress(ys[0], sides[0])
        want_dec = codec.decompress(want_enc["strings"], want_enc["shape"], sides[0])["y_hat"]
        assert codec_key(want_enc) != codec_key(codec.compress(ys[1], sides[1]))
        with pending(s1, delay, [ys[0], sides[0]], [ys[1], sides[1]]) as (yb, sb):
            enc = codec.compress(yb, sb)
        assert codec_key(enc) == codec_key(want_enc)
        with pending(s2, delay, [sides[0]], [sides[1]]) as (sb,):
            dec = codec.decompress(enc["strings"], enc["shape"], sb)["y_hat"]
        assert torch.equal(dec, want_dec) and torch.equal(dec, want_enc["y_hat"])


# ---- e. the raw probes -------------------------------------------------------------------------------------------------------------
def _probe_inputs(seed):
    """every latent of a 16 x 16 x 16 item as (n, 4) rows (no channel left out: the true and the decoy rows are equally many)"""
    y, sg, mu, pi = T.make_latent(seed, 16, 16, 16)
    sym = T.torch_int(np.round(y).reshape(-1))
    return [dv(sym)] + [dv(p.reshape(4, -1).T) for p in (sg, mu, pi)], int(np.abs(sym).max()) + 1


def _probes(mode_id, max_bs):
    """name -> f(stream handle, v, s, m, w) -> comparable result (device outputs allocated, poisoned, on the current stream)"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    import ctypes as C

    def symtab(st, v, s, m, w):
        out = torch.full((v.numel(),), -1, dtype=torch.int32, device=DEV)
        _lib.check(L.fgmm_build_symtab_hip(ctx, st, v.data_ptr(), s.data_ptr(), m.data_ptr(), w.data_ptr(), v.numel(), s.stride(0), s.stride(1), mode_id, out.data_ptr()))
        return [out]

    def cdf(st, v, s, m, w):
        c1, c2 = (torch.full((v.numel(),), -1.0, dtype=torch.float32, device=DEV) for _ in range(2))
        _lib.check(L.fgmm_gmm_cdf_hip(ctx, st, v.data_ptr(), s.data_ptr(), m.data_ptr(), w.data_ptr(), v.numel(), s.stride(0), s.stride(1), mode_id, c1.data_ptr(),
                                      c2.data_ptr()))
        return [c1, c2]

    def softmax4(st, v, s, m, w):  # (the means as logits)
        out = torch.full_like(m, -1.0)
        _lib.check(L.fgmm_softmax4_hip(ctx, st, m.data_ptr(), out.data_ptr(), m.size(0)))
        return [out]

    def tab(st, v, s, m, w):
        n, form = s.size(0), hdr_form(max_bs)
        cap = n * (2 * (2 * max_bs + 2) + 4)
        hdr = torch.zeros(n * form, dtype=torch.uint8, device=DEV)
        blk_off = torch.zeros(n // 16 + 2, dtype=torch.int32, device=DEV)
        rows = torch.zeros(cap + 128, dtype=torch.uint8, device=DEV)
        used = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        tl = C.c_int32(0)
        _lib.check(L.fgmm_build_tab_hip(ctx, st, s.data_ptr(), m.data_ptr(), w.data_ptr(), n, s.stride(0), s.stride(1), mode_id, max_bs, 0, hdr.data_ptr(),
                                        blk_off.data_ptr(), rows.data_ptr(), cap, used.data_ptr(), C.byref(tl)))
        return [hdr, blk_off, rows, used[:1], torch.tensor([tl.value])]

    def symtab_bits(st, v, s, m, w):  # (v: a packed table here)
        cost = torch.full((v.numel(),), -1, dtype=torch.int32, device=DEV)
        tot = torch.full((2,), 77, dtype=torch.int64, device=DEV)
        _lib.check(L.fgmm_symtab_bits_hip(ctx, st, v.data_ptr(), None, v.numel(), cost.data_ptr(), tot.data_ptr(), tot.data_ptr() + 8))
        return [cost, tot]

    return {"fgmm_build_symtab_hip": symtab, "fgmm_gmm_cdf_hip": cdf, "fgmm_softmax4_hip": softmax4, "fgmm_build_tab_hip": tab, "fgmm_symtab_bits_hip": symtab_bits}


def _table(outs, max_bs):
    """what fgmm_build_tab_hip's outputs stand for (its blocks are placed in arrival order: the bytes differ from run to run)"""
    hdr, blk_off, rows, used, tl = (o.cpu().numpy() for o in outs)
    dt = {2: np.uint16, 4: np.uint32, 8: np.uint64}[hdr_form(max_bs)]
    nblk = (len(hdr.view(dt)) + int(tl[0]) - 1) // int(tl[0])
    return expand_trimmed(hdr.view(dt), rows, max_bs, blk_off.view(np.uint32)[:nblk], int(tl[0])), int(used[0])


@pytest.mark.parametrize("name", ["fgmm_build_symtab_hip", "fgmm_gmm_cdf_hip", "fgmm_softmax4_hip", "fgmm_build_tab_hip", "fgmm_symtab_bits_hip"])
def test_raw_probes_on_a_callers_stream(streams, delay, name):
    s1, s2, third = streams
    mode_id = _lib.mode_id("polya")
    (true, bs_t), (decoy, bs_d) = _probe_inputs(9500), _probe_inputs(9501)
    max_bs = max(bs_t, bs_d)
    f = _probes(mode_id, max_bs)[name]
    if name == "fgmm_symtab_bits_hip":  # its input is a table: the true rows' and the decoy rows'
        torch.cuda.synchronize()
        true, decoy = ([_probes(mode_id, max_bs)["fgmm_build_symtab_hip"](None, *t)[0]] + t[1:] for t in (true, decoy))
    torch.cuda.synchronize()
    want, other = f(None, *true), f(None, *decoy)
    torch.cuda.synchronize()
    with pending(s1, delay, true, decoy) as t:
        got = f(s1.cuda_stream, *t)
        got_3 = snapshot(third, got)
    if name == "fgmm_build_tab_hip":
        (tw, uw), (to, _) = _table(want, max_bs), _table(other, max_bs)
        assert not np.array_equal(tw, to)
        for g in (got, got_3):
            tg, ug = _table(g, max_bs)
            assert np.array_equal(tg, tw) and ug == uw
    else:
        assert not same(want, other)
        assert same(got, want) and same(got_3, want)


# ---- f. checkerboard split and merge: stream-ordered, not complete on return ------------------------------------------------------------
def test_checkerboard_split_and_merge_are_stream_ordered(streams, delay):
    from flashgmm_amd.ops import ckbd_embed, ckbd_unembed

    s1, s2, third = streams
    g = torch.Generator().manual_seed(96)
    y, y_d = ((torch.randn((1, 6, 8, 12), generator=g) * 50).to(DEV) for _ in range(2))
    want = torch.stack([_take(y, True), _take(y, False)])
    assert not torch.equal(want, torch.stack([_take(y_d, True), _take(y_d, False)]))
    with pending(s1, delay, [y], [y_d]) as (yb,):
        halves = ckbd_unembed(yb, "even")
        back = ckbd_embed(halves, "even")
        done = torch.cuda.Event()
        done.record()
        # consumed on the same stream
        assert torch.equal(halves, want) and torch.equal(back, y)
        # consumed on another stream, behind an event recorded on the caller's
        with torch.cuda.stream(s2):
            s2.wait_event(done)
            h2, b2 = halves.clone(), back.clone()
        s2.synchronize()
    assert torch.equal(h2, want) and torch.equal(b2, y)


def _take(y, anchors):
    """the checkerboard half of y [n, c, h, w] -> [n, c, h, w/2] by slicing (anchor parity "even": anchors where row + column is even)"""
    out = y.new_zeros(y.shape[:3] + (y.shape[3] // 2,))
    a, b = (0, 1) if anchors else (1, 0)
    out[..., 0::2, :] = y[..., 0::2, a::2]
    out[..., 1::2, :] = y[..., 1::2, b::2]
    return out


# ---- g. two streams, one thread ----------------------------------------------------------------------------------------------------
def test_calls_alternating_between_two_streams_share_the_workspace(oracle, streams, delay):
    s1, s2, third = streams
    gmc = GaussianMixtureConditional(K=4, mode="polya")
    lat = [T.make_latent(9700 + i, 16, 16, 16, zero_frac=0.2) for i in range(2)]
    t = [[dv(a) for a in l] for l in lat]
    want = [oracle_bytes(oracle, "polya", *l) for l in lat]
    want_q = [key(gmc.quantize_rdo(*x, 0.5, per_channel=True)) for x in t]
    assert want[0][0] != want[1][0] and want_q[0] != want_q[1]
    for rnd in range(5):
        for k, s in ((0, s1), (1, s2)):  # (each stream's decoy is the other stream's true input)
            with pending(s, delay, t[k], t[1 - k]) as p:
                (b, am, zb), yq = gmc.compress(*p)
                (yq_3,) = snapshot(third, [yq])
            assert b == want[k][0] and am == want[k][1] and np.array_equal(yq_3.cpu().numpy(), want[k][3]), (rnd, k)
            zb = zb.cpu()  # (a bitmap on the device is fetched through the caller's stream before the native call: that would wait for the producer)
            with pending(s, delay, t[k][1:], t[1 - k][1:]) as p:
                y_hat = gmc.decompress(b, am, zb, *p)
                (y_hat_3,) = snapshot(third, [y_hat])
            assert np.array_equal(y_hat_3.cpu().numpy(), want[k][3]) and torch.equal(y_hat, y_hat_3), (rnd, k)
            with pending(s, delay, t[k], t[1 - k]) as p:
                q = gmc.quantize_rdo(*p, 0.5, per_channel=True)
                (q_3,) = snapshot(third, [q.y])
            assert key(q) == want_q[k] and q_3.cpu().numpy().tobytes() == want_q[k][0], (rnd, k)


# ---- h. four threads, four streams -------------------------------------------------------------------------------------------------
def test_concurrent_callers_each_on_a_stream_of_their_own(oracle, streams, delay):
    third = streams[2]
    cases = []
    for seed in range(4):
        lat = T.make_latent(9800 + seed, M=16, h=12, w=8)
        cases.append(([dv(a) for a in lat], oracle_bytes(oracle, "polya", *lat)))
    assert len({c[1][0] for c in cases}) == 4
    own = [torch.cuda.Stream(DEV) for _ in range(4)]
    errors = []
    # Between queueing its producer and making its call a thread may have to wait for the interpreter lock: up to the switch interval
    # (5 ms) for each of the three other threads.  The producers here are therefore 4 * DELAY_MS long, twice that bound.
    start = threading.Barrier(4)
    torch.cuda.synchronize()

    def worker(k):
        try:
            gmc = GaussianMixtureConditional(K=4, mode="polya")
            t, (want, am_w, _, yq_w) = cases[k]
            d = cases[(k + 1) % 4][0]  # the decoy: the next thread's input
            start.wait()
            for it in range(5):
                with pending(own[k], delay, t, d, times=4) as p:
                    (b, am, zb), yq = gmc.compress(*p)
                    (yq_3,) = snapshot(third, [yq])
                assert b == want and am == am_w and np.array_equal(yq_3.cpu().numpy(), yq_w), it
                zb = zb.cpu()  # (see the test above)
                with pending(own[k], delay, t[1:], d[1:], times=4) as p:
                    y_hat = gmc.decompress(b, am, zb, *p)
                    (y_hat_3,) = snapshot(third, [y_hat])
                assert np.array_equal(y_hat_3.cpu().numpy(), yq_w) and torch.equal(y_hat, y_hat_3), it
        except BaseException as e:  # pragma: no cover
            start.abort()
            errors.append((k, repr(e)))

    th = [threading.Thread(target=worker, args=(k,)) for k in range(4)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errors, errors


# ---- i. the latent codecs ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lam", [0.0, 0.5])
@pytest.mark.parametrize("kind", ["ckbd", "groups"])
def test_latent_codecs_under_a_side_stream(streams, delay, kind, lam):
    """CheckerboardLatentCodec / ChannelGroupsLatentCodec on the exact networks of tests/synth.py, at the sizes of the codec parity
    test (tests/golden/make_golden.py G7_CKBD / G7_GROUPS)"""
    from flashgmm_amd.latent_codecs import ChannelGroupsLatentCodec, CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec

    s1, s2, third = streams
    Ctx, Par = T.exact_modules()
    gmm = lambda: GaussianMixtureConditionalLatentCodec(K=4, quantizer="noise", mode="polya")  # noqa: E731
    if kind == "ckbd":
        c, c_side, h, w = 6, 8, 8, 12
        codec = CheckerboardLatentCodec(latent_codec={"y": gmm()}, context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c),
                                        anchor_parity="even", rdo_lambda=lam).cuda()
    else:
        groups, c_side, h, w = [2, 2, 4], 8, 8, 12
        c = sum(groups)
        latent = {f"y{k}": CheckerboardLatentCodec(latent_codec={"y": gmm()}, context_prediction=Ctx(g, 2 * g),
                                                   entropy_parameters=Par(2 * g + (k > 0) * 2 * g + c_side, g), rdo_lambda=lam) for k, g in enumerate(groups)}
        chctx = {f"y{k}": Ctx(sum(groups[:k]), 2 * groups[k]) for k in range(1, len(groups))}
        codec = ChannelGroupsLatentCodec(groups=groups, channel_context=chctx, latent_codec=latent).cuda()
    (y, side), (y_d, side_d) = ([dv(a) for a in T.exact_codec_inputs(9900 + i, c, c_side, h, w)] for i in range(2))
    want_enc = codec.compress(y, side)
    want_dec = codec.decompress(want_enc["strings"], want_enc["shape"], side)["y_hat"]
    assert codec_key(want_enc)[0] != codec_key(codec.compress(y_d, side_d))[0]
    if lam:
        assert not torch.equal(want_enc["y_hat"], torch.round(y))  # (RDOQ moved something)
    with pending(s1, delay, [y, side], [y_d, side_d]) as (yb, sb):
        enc = codec.compress(yb, sb)
    assert codec_key(enc) == codec_key(want_enc)
    with pending(s2, delay, [side], [side_d]) as (sb,):
        dec = codec.decompress(enc["strings"], enc["shape"], sb)["y_hat"]
    assert torch.equal(dec, want_dec)
