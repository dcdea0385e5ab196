"""GPU (-m gpu): segdec_kernel at its STRUCTURAL edges - window lengths around the plain | slow boundary and the slow search's pass
boundaries, batches that fill, overrun and underrun the 2048-edge LDS budget, the producers' seam, short last segments, channels
of 1 .. 257 latents under every layout of dead channels, bypass escapes at the first and last symbol of a stream, a segment and a
batch - on the corpus of tests/segdec_ref.py (whose properties tests/test_segdec_ref_cpu.py pins without a GPU).

The expected symbols are the CPU oracle's (oracle.decode_gmm), element for element, never the table path's.  The fallback hides
errors - a segment the kernel gets wrong fails its note and the table path decodes the item again - so every test also asserts
``(ctx_stat(0, 4), ctx_stat(0, 5)) == (1, 0)``: the kernel settled the item ITSELF.  The last segment has no note at all; it is
compared on its own.

What equality with the oracle cannot see, by the kernel's design: HOW a segment is cut into batches (a planner that stops one
latent short of a full budget decodes the same symbols into the same notes) and WHICH of the two searches a 64-edge window gets
(both are exact there for every cf a valid stream holds: tests/test_segdec_ref_cpu.py,
test_outermost_window_edges_are_saturated_even_where_the_rounding_is_tight).  The corpus pins those boundaries by decoding both
sides of them; a change that breaks either side - a wrong lane mask, a seam compared across two latents - fails here."""
import functools

import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, _lib
from tests import segdec_ref as S
from tests import synth as T

pytestmark = pytest.mark.gpu

MODES = list(S.MODES)
DEV = "cuda:0"
KIN = ("ladder_63", "ladder_128", "budget", "full_width", "full_width_short", "extremes", "bypass_at")
FILLER_SHAPE = (228, 64, 86)  # 192 of its channels are coded: 1 056 768 latents, 4128 segments at stride 256 - the two-wave launch


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
def corpus(mode):
    return {
        "ladder_63": S.ladder(1, 56, 72, 16, mode),
        "ladder_128": S.ladder(2, 120, 136, 16, mode),
        "budget": S.budget(3, mode),
        "full_width": S.full_width(4),
        "full_width_short": S.full_width(5, abs_max=25),
        "extremes": S.extremes(6, mode),
        "bypass_at": S.bypass_at(7),
    }


def stat():
    return _lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5)


class Case:
    """one item on the device with everything the oracle says about it: the planes as the codec gets them (fp32 or fp16), the rows
    widened to float32 for the oracle, its bytes and its symbols"""

    def __init__(self, oracle, mode, it, stride=256, clamp=True, f16=False):
        y, sg, mu, pi = it
        if f16:
            sg, mu, pi = T.to_float16_planes(sg, mu, pi)
        self.mode, self.stride, self.clamp = mode, stride, clamp
        self.t = [dv(a) for a in (y, sg, mu, pi)]
        wide = (y, *(np.asarray(a, np.float32) for a in (sg, mu, pi)))
        self.sym, s, m, w, self.am, self.zb = S.coded(wide, clamp=clamp)
        self.n = len(self.sym)
        self.want_bytes = oracle.encode_gmm(mode, self.sym, s, m, w)
        self.want_sym = oracle.decode_gmm(mode, self.want_bytes, s, m, w, self.am + 1)
        self.yq = np.rint(y)
        self.plain = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
        self.ck = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp, checkpoint_stride=stride)
        self.enc = None

    def compress(self):
        """1. with and without checkpoints: the same bytes, the oracle's; a note every `stride` symbols"""
        if self.enc is None:
            (b0, am0, zb0), _ = self.plain.compress(*self.t)
            (b1, am1, zb1), yq1 = self.ck.compress(*self.t)
            assert type(b0) is bytes and isinstance(b1, CheckpointedBytes)
            assert b0 == self.want_bytes and bytes(b1) == self.want_bytes
            assert am0 == am1 == self.am and zb0.cpu().tolist() == zb1.cpu().tolist() == self.zb.tolist()
            assert len(b1.ckpt) == (self.n - 1) // self.stride and b1.ckpt_stride == self.stride
            assert np.array_equal(yq1.cpu().numpy(), self.yq)
            self.enc = (b1, am1, zb1)
        return self.enc

    def check(self, y_hat, what):
        """2. the oracle's symbols element for element; the last segment - which no note verifies - on its own"""
        got = y_hat.cpu().numpy()
        live = np.nonzero(self.zb)[0]
        sym = got[0, live].reshape(-1)
        last = (self.n - 1) // self.stride * self.stride
        want = self.want_sym.astype(np.float32)
        bad = np.nonzero(sym[:last] != want[:last])[0]
        assert bad.size == 0, (f"{what}: {bad.size} symbols differ from the oracle's, the first at {bad[:5]} "
                               f"(segment {bad[0] // self.stride})")
        bad = np.nonzero(sym[last:] != want[last:])[0]
        assert bad.size == 0, (f"{what}: the LAST segment [{last}, {self.n}) - checked against no note - differs from the oracle's at "
                               f"{(bad[:5] + last)}: got {sym[last:][bad[:5]]}, want {want[last:][bad[:5]]}")
        assert np.array_equal(self.want_sym, self.sym), what
        assert not got[0, np.nonzero(self.zb == 0)[0]].any(), f"{what}: a dead channel is not zero"

    def decode_alone(self, what, expect=(1, 0)):
        """-> y_hat of the item decoded in a call of its own (gpu_decode must be 1), 3. settled by the kernel itself"""
        b, am, zb = self.compress()
        y_hat = self.ck.decompress(b, am, zb, *self.t[1:])
        st = stat()
        self.check(y_hat, what)
        assert st == expect, f"{what}: (settled by the segment decoder, handed back) = {st}"
        return y_hat


@functools.lru_cache(maxsize=None)
def case(oracle, mode, name):
    return Case(oracle, mode, corpus(mode)[name])


@functools.lru_cache(maxsize=None)
def alone(oracle, mode, name):
    """the three-wave result of a corpus item decoded alone (gpu_decode = 1 set by the caller)"""
    return case(oracle, mode, name).decode_alone(f"{mode} {name}")


@pytest.mark.parametrize("name", KIN)
@pytest.mark.parametrize("mode", MODES)
def test_corpus_item_alone_is_the_oracles_and_settled_by_the_kernel(oracle, ctx_options, mode, name):
    """every corpus item on its own: bytes, notes, the oracle's symbols, the last segment, and (1, 0) - full_width too: in a valid
    stream cf is never below F[0], so the slow search's `J < 0` hand-back must not trigger"""
    ctx_options(gpu_decode=1)
    alone(oracle, mode, name)


@pytest.mark.parametrize("mode", MODES)
def test_corpus_items_in_one_batch_equal_themselves_alone(oracle, ctx_options, mode):
    """4. the kin in ONE call (one launch, segments of all items ordered heaviest first) against each item alone"""
    ctx_options(gpu_decode=1)
    cs = [case(oracle, mode, name) for name in KIN]
    single = [alone(oracle, mode, name) for name in KIN]
    encs = [c.compress() for c in cs]
    out = cs[0].ck.decompress_batch([e[0] for e in encs], [e[1] for e in encs], [e[2] for e in encs],
                                    *([c.t[k] for c in cs] for k in (1, 2, 3)))
    assert stat() == (len(KIN), 0)
    for c, name, o, a in zip(cs, KIN, out, single):
        c.check(o, f"{mode} {name} in a batch")
        assert torch.equal(o, a), name


@pytest.mark.parametrize("f16,clamp", [(True, True), (False, False), (True, False)])
@pytest.mark.parametrize("name", ("ladder_63", "ladder_128", "budget"))
@pytest.mark.parametrize("mode", MODES)
def test_fp16_planes_and_unclamped_sigma(oracle, ctx_options, mode, name, f16, clamp):
    """the other three instantiations of the kernel (fp16 planes: the oracle gets the widened values; clamp_scales=False: the IEEE
    evaluation of every edge, sigma far above 0.05) on the window-length and budget corpora"""
    ctx_options(gpu_decode=1)
    Case(oracle, mode, corpus(mode)[name], clamp=clamp, f16=f16).decode_alone(f"{mode} {name} f16={f16} clamp={clamp}")


@pytest.mark.parametrize("stride", (256, 512, 2048))
@pytest.mark.parametrize("mode", MODES)
def test_segment_residues_channel_sizes_and_dead_channels(oracle, ctx_options, mode, stride):
    """shapes(): every residue of n against the stride (last segments of 1, 2, 63, 64, 65, 255 and `stride` symbols, a single symbol
    after the only note), channels smaller than a batch, dead channels in every layout (the live-then-dead list, segzero_kernel)"""
    ctx_options(gpu_decode=1)
    for k, shape in enumerate(S.shapes(stride)):
        c = Case(oracle, mode, S.shape_item(20 + k, shape), stride=stride)
        assert c.n == S.live_count(shape) > stride
        c.decode_alone(f"{mode} stride {stride} shape {shape} (n = {c.n} = {c.n // stride} * {stride} + {c.n % stride})")


def _resampled(b, n, stride):
    """the notes of a stride-256 encode taken (or repeated) at multiples of `stride`: right wherever 256 divides the position"""
    ck = b.ckpt
    idx = [min(max((k * stride) // 256 - 1, 0), len(ck) - 1) for k in range(1, (n - 1) // stride + 1)]
    return CheckpointedBytes(bytes(b), ck[idx].copy(), stride)


@pytest.mark.parametrize("mode", MODES)
def test_items_that_are_not_the_kernels_never_reach_it(oracle, ctx_options, mode):
    """gpu_decodable(): a stride that is no power of two or below 256, a stream without a note (n <= stride), abs_max = 1023
    (2 * 1024 + 2 edges > 2048): the same y_hat, and neither counter moves"""
    ctx_options(gpu_decode=1)
    c = case(oracle, mode, "bypass_at")
    b, am, zb = c.compress()
    for stride in (128, 384):
        odd = _resampled(b, c.n, stride)
        assert len(odd.ckpt) == (c.n - 1) // stride
        y_hat = c.ck.decompress(odd, am, zb, *c.t[1:])
        assert stat() == (0, 0), stride
        c.check(y_hat, f"{mode} stride {stride}")
    for shape in ((256, 1, 1, "none"), (1, 8, 25, "none")):  # n == stride; n < stride
        s = Case(oracle, mode, S.shape_item(60, shape))
        sb, sam, szb = s.compress()
        assert len(sb.ckpt) == 0
        y_hat = s.ck.decompress(sb, sam, szb, *s.t[1:])
        assert stat() == (0, 0), shape
        s.check(y_hat, f"{mode} {shape}")
    y, sg, mu, pi = corpus(mode)["budget"]
    y = y.copy()
    y.reshape(-1)[-1] = np.float32(1022.25)
    wide = Case(oracle, mode, (y, sg, mu, pi))
    assert wide.am == 1023
    wb, wam, wzb = wide.compress()
    assert len(wb.ckpt) == 14
    y_hat = wide.ck.decompress(wb, wam, wzb, *wide.t[1:])
    assert stat() == (0, 0)
    wide.check(y_hat, f"{mode} abs_max 1023")
    assert case(oracle, mode, "budget").am == 1022  # ... and one less is the kernel's: test_corpus_item_alone[budget]


@functools.lru_cache(maxsize=None)
def filler():
    """ordinary latents, built once per module: enough segments to push a call past 4096"""
    M, h, w = FILLER_SHAPE
    return [dv(a) for a in T.make_latent(900, M=M, h=h, w=w)]


@pytest.mark.parametrize("mode", MODES)
def test_two_wave_launch_decodes_the_edge_items_as_the_three_wave_launch_does(oracle, ctx_options, mode):
    """a call of more than 4096 segments takes the launch shape with ONE producer (blockDim == 128: no seam, no second handshake; the
    threshold is launch_segdec's `n_segs <= 4096 ? 192 : 128` in fgmm_tab.hip - if it moves, FILLER_SHAPE has to move with it):
    the edge items next to a filler of 4128 segments are settled there too, equal to their three-wave results and the oracle's; the
    filler equals what the table path makes of the same bytes without their notes"""
    ctx_options(gpu_decode=1)
    names = ("ladder_63", "ladder_128", "budget", "bypass_at")
    cs = [case(oracle, mode, name) for name in names]
    three = [alone(oracle, mode, name) for name in names]
    t = filler()
    ck = cs[0].ck
    (fb, fam, fzb), fyq = ck.compress(*t)
    encs = [c.compress() for c in cs] + [(fb, fam, fzb)]
    n_segs = sum(len(e[0].ckpt) + 1 for e in encs)
    assert n_segs > 4096 >= n_segs - (len(fb.ckpt) + 1)  # past the threshold only with the filler
    out = ck.decompress_batch([e[0] for e in encs], [e[1] for e in encs], [e[2] for e in encs],
                              *([c.t[k] for c in cs] + [t[k]] for k in (1, 2, 3)))
    assert stat() == (len(encs), 0)
    for c, name, o, a in zip(cs, names, out, three):
        c.check(o, f"{mode} {name} in the two-wave launch")
        assert torch.equal(o, a), name
    ctx_options(gpu_decode=0)
    want = cs[0].plain.decompress(bytes(fb), fam, fzb, *t[1:])
    assert stat() == (0, 0)
    assert torch.equal(out[-1], want) and torch.equal(want, fyq)


@pytest.mark.parametrize("mode", MODES)
def test_heaviest_first_order_changes_nothing_but_the_order(oracle, ctx_options, mode):
    """two copies of one item in a call; the first copy's first half is made very cheap (a word of the stream every few hundred
    symbols), so its segments rank last and the second copy's - notes untouched - are interleaved with the rest: the same results,
    all settled"""
    ctx_options(gpu_decode=1)
    c = case(oracle, mode, "bypass_at")
    cheap = Case(oracle, mode, S.cheap_copy(corpus(mode)["bypass_at"], 1024))
    b, am, zb = c.compress()
    cb, cam, czb = cheap.compress()
    words = np.diff(np.concatenate([[0], cb.ckpt["pos"].astype(np.int64)]))
    assert words[:4].max() < np.diff(b.ckpt["pos"].astype(np.int64)).min()  # the ranking really is another one
    for order in ((cheap, c), (c, cheap), (c, c)):
        encs = [x.compress() for x in order]
        out = c.ck.decompress_batch([e[0] for e in encs], [e[1] for e in encs], [e[2] for e in encs],
                                    *([x.t[k] for x in order] for k in (1, 2, 3)))
        assert stat() == (2, 0)
        for x, o in zip(order, out):
            x.check(o, f"{mode} {'cheap' if x is cheap else 'plain'} copy")
            if x is c:
                assert torch.equal(o, alone(oracle, mode, "bypass_at"))
