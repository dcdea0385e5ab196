"""GPU (-m gpu): every symbol of every row through the production coder paths - the sweep items of tests/sweep_ref.py (whose
properties tests/test_sweep_ref_cpu.py pins without a GPU) coded and decoded by ``compress_batch`` / ``decompress_batch`` under
every decode-table configuration, plane type and launch mix, by the GPU segment decoder, priced by the rate kernel, and their rows
built by the two table building blocks at every block size.

A decoded symbol v consults F[v] and F[v + 1] of its row and rANS advances its state with them, so a sweep item that decodes to the
oracle's symbols has every entry F_i[v], v in [-A, A + 1], of every row right in the configuration that decoded it.  Expected values
are always the CPU oracle's, computed here and never stored - oracle.encode_gmm bytes, oracle.decode_gmm symbols element for
element, oracle.cdftab tables - and every comparison is exact equality.  A failure names the first differing (parameter set,
symbol) pair, recovered from the flat index through the item's arrangement."""
import functools

import numpy as np
import pytest
import torch

from flashgmm_amd import CheckpointedBytes, GaussianMixtureConditional, _lib
from tests import helpers
from tests import rate_ref as R
from tests import sweep_ref as W
from tests import synth as T
from tests.test_gpu_parity import gpu_cdftab, gpu_tab

pytestmark = pytest.mark.gpu

MODES = list(W.MODES)
AS = list(W.HALF_WIDTHS)
DEV = "cuda:0"
STRIDE = 256
FGMM_TAB_CLAMP, FGMM_TAB_RAW_ROWS = 2, 4


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bf(bits):
    """bfloat16 bit patterns -> a device tensor of that dtype"""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).to(DEV).view(torch.bfloat16)


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


def softmax_dev(logit_planes):
    """the device's own pi for logits (fgmm_softmax4_hip: the kernels' fixed binary32 sequence), as planes"""
    L, ctx = _lib.lib(), _lib.ctx(0)
    rows = dv(logit_planes.reshape(4, -1).T)
    out = torch.empty_like(rows)
    torch.cuda.synchronize()
    _lib.check(L.fgmm_softmax4_hip(ctx, None, rows.data_ptr(), out.data_ptr(), rows.size(0)))
    return np.ascontiguousarray(out.cpu().numpy().T).reshape(logit_planes.shape)


def stat():
    return _lib.ctx_stat(0, 4), _lib.ctx_stat(0, 5)


class Item:
    """one item on the device with everything the oracle says about it.  ``pairs`` = (set, symbol) of every coded latent in coding
    order, ``kinds`` the family of each set; ``planes``: "f32", "f16", "bf16" (the oracle is fed the widened values) or "logits"
    (float32 planes, the weights as log(pi): the oracle is fed the device's own softmax)"""

    def __init__(self, oracle, mode, name, it, pairs, kinds, clamp=True, planes="f32"):
        y, sg, mu, pi = it
        self.mode, self.name, self.clamp, self.logits = mode, name, clamp, planes == "logits"
        self.pairs, self.kinds = pairs, kinds
        if planes == "f16":
            r, wide = W.planes((sg, mu, pi), "f16")
            p = [dv(a) for a in r]
        elif planes == "bf16":
            r, wide = W.planes((sg, mu, pi), "bf16")
            p = [bf(a) for a in r]
        elif planes == "logits":
            lg = np.log(pi).astype(np.float32)
            p, wide = [dv(sg), dv(mu), dv(lg)], (sg, mu, softmax_dev(lg))
        else:
            p, wide = [dv(sg), dv(mu), dv(pi)], (sg, mu, pi)
        self.t = [dv(y)] + p
        self.sym, s, m, w, self.am, self.zb, self.yq = T.to_coder_inputs(y, *wide, clamp=clamp)
        self.rows = tuple(np.ascontiguousarray(a, np.float32) for a in (s, m, w))
        self.n = len(self.sym)
        self.want_bytes = oracle.encode_gmm(mode, self.sym, *self.rows)
        self.want_sym = oracle.decode_gmm(mode, self.want_bytes, *self.rows, self.am + 1)
        self.gmc = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp)
        self.ck = GaussianMixtureConditional(K=4, mode=mode, clamp_scales=clamp, checkpoint_stride=STRIDE)
        self._enc = {}

    def where(self, i):
        """flat index in coding order -> the (parameter set, symbol) it codes"""
        if self.pairs is None:
            return f"latent {int(i)}"
        p, v = int(self.pairs[0][i]), int(self.pairs[1][i])
        return f"latent {int(i)}: set {p} ({self.kinds[p]}), symbol {v}"

    def check_enc(self, enc, what):
        b, am, zb = enc
        assert am == self.am and zb.cpu().tolist() == self.zb.tolist(), f"{what} {self.name}: abs_max {am} / zero bitmap differ"
        b = bytes(b)
        if b != self.want_bytes:
            n = min(len(b), len(self.want_bytes))
            d = np.nonzero(np.frombuffer(b[:n], np.uint8) != np.frombuffer(self.want_bytes[:n], np.uint8))[0]
            raise AssertionError(f"{what} {self.name}: {len(b)} bytes against the oracle's {len(self.want_bytes)}, the last differing "
                                 f"byte at {int(d[-1]) if d.size else n} (the stream is written back to front)")

    def compress(self, ck=False):
        """-> (bytes, abs_max, zero_bitmap) of the item coded in a call of its own, the oracle's"""
        if ck not in self._enc:
            codec = self.ck if ck else self.gmc
            enc, yq = codec.compress(*self.t, weights_are_logits=self.logits)
            self.check_enc(enc, "compress")
            assert np.array_equal(yq.cpu().numpy(), self.yq), self.name
            if ck:
                assert isinstance(enc[0], CheckpointedBytes) and len(enc[0].ckpt) == (self.n - 1) // STRIDE
            self._enc[ck] = enc
        return self._enc[ck]

    def check(self, y_hat, what, want_y=True, last_from=None):
        """the oracle's symbols element for element (and round(y), where the oracle itself decodes the coded symbols); dead channels
        zero; with last_from the symbols from there on - the segment no note verifies - are compared on their own"""
        got = y_hat.cpu().numpy()
        assert got.shape == self.yq.shape, (what, got.shape)
        sym = got[0, np.nonzero(self.zb)[0]].reshape(-1)
        want = self.want_sym.astype(np.float32)
        cut = self.n if last_from is None else last_from
        bad = np.nonzero(sym[:cut] != want[:cut])[0]
        assert bad.size == 0, (f"{what} {self.name}: {bad.size} symbols differ from the oracle's, the first at {self.where(bad[0])}: "
                               f"got {sym[bad[0]]}, want {want[bad[0]]}")
        bad = np.nonzero(sym[cut:] != want[cut:])[0] + cut
        assert bad.size == 0, (f"{what} {self.name}: the LAST segment [{cut}, {self.n}) differs from the oracle's, first at "
                               f"{self.where(bad[0])}: got {sym[bad[0]]}, want {want[bad[0]]}")
        assert not got[0, np.nonzero(self.zb == 0)[0]].any(), f"{what} {self.name}: a dead channel is not zero"
        if want_y:
            assert np.array_equal(self.want_sym, self.sym) and np.array_equal(got, self.yq), f"{what} {self.name}"

    def decode(self, what, ck=False, **kw):
        b, am, zb = self.compress(ck)
        y_hat = (self.ck if ck else self.gmc).decompress(b, am, zb, *self.t[1:], weights_are_logits=self.logits)
        self.check(y_hat, what, **kw)
        return y_hat


def batch(items, ck=False):
    """the items coded in ONE call and decoded in one -> [y_hat]; every item's bytes are the oracle's"""
    codec = items[0].ck if ck else items[0].gmc
    res = codec.compress_batch(*([x.t[k] for x in items] for k in range(4)))
    for x, (enc, yq) in zip(items, res):
        x.check_enc(enc, "compress_batch")
        assert np.array_equal(yq.cpu().numpy(), x.yq), x.name
    return res, codec.decompress_batch([r[0][0] for r in res], [r[0][1] for r in res], [r[0][2] for r in res],
                                       *([x.t[k] for x in items] for k in (1, 2, 3)))


@functools.lru_cache(maxsize=None)
def item(oracle, mode, A, which, clamp=True, planes="f32", P=W.P_SETS):
    """which: "sweep" | "by_channel" (the monotone ladder) | "nonmono" (the sets with a negative weight, sweep arrangement)"""
    if which == "nonmono":
        sets, kinds = W.nonmono_sets(P), ("nonmono",) * P
    else:
        sets, kinds = W.ladder(mode, P), W.ladder_kinds(mode, P)
    if which == "by_channel":
        it, pairs = W.sweep_item_by_channel(sets, A), W.by_channel_pairs(P, A)
    else:
        it, pairs = W.sweep_item(sets, A), W.sweep_pairs(P, A)
    x = Item(oracle, mode, f"{mode} A={A} {which} clamp={clamp} {planes} P={P}", it, pairs, kinds, clamp, planes)
    assert x.am == A and np.array_equal(x.sym, pairs[1])
    return x


# ---- a. production round trip ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clamp", [True, False])
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_production_round_trip(oracle, mode, A, clamp):
    """compress_batch / decompress_batch at their defaults: the oracle's bytes, abs_max == A, the zero bitmap; y_hat == round(y), the
    dead channels zero - the sweep item and its transposed arrangement"""
    items = [item(oracle, mode, A, which, clamp) for which in ("sweep", "by_channel")]
    res, out = batch(items)
    for x, (enc, _), o in zip(items, res, out):
        assert enc[1] == A
        x.check(o, "decompress_batch")
    assert items[0].zb.tolist().count(0) == 2


# ---- b. every table configuration -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_every_table_configuration_decodes_it(oracle, ctx_options, mode, A):
    """one compressed pair of items decoded with Elias-Fano rows from 14, 33 and 49 entries on (ef_rows = 1 forces them whatever the
    decoder count) and with uint16 rows only, each at blocks of 16, 48 and 128 latents; by the generic kernels; in 1 and 7 pieces;
    through the overflow re-run of a 1 MB staging area: the same symbols every time, the oracle's"""
    items = [item(oracle, mode, A, which) for which in ("sweep", "by_channel")]
    encs = [x.compress() for x in items]
    args = ([e[0] for e in encs], [e[1] for e in encs], [e[2] for e in encs], *([x.t[k] for x in items] for k in (1, 2, 3)))

    def decode(tag):
        for x, o in zip(items, items[0].gmc.decompress_batch(*args)):
            x.check(o, tag)

    cap0 = _lib.get_option(0, "tab_cap_e")
    assert cap0 == W.CAP_DEFAULT
    _lib.set_profiling(0, True)  # the table kernel counts the edges it evaluates only for a profiling caller
    try:
        for cap in W.caps(A):
            assert W.tab_tl(A + 1, cap) in (16, 48, 128)
            for ef_rows, ef_min in ((1, 14), (1, 33), (1, 49), (2, 33)):
                ctx_options(tab_cap_e=cap, ef_rows=ef_rows, ef_min=ef_min)
                decode(f"tab_cap_e={cap} ef_rows={ef_rows} ef_min={ef_min}")
        assert _lib.ctx_stat(0, 3) > 0
        ctx_options(tab_cap_e=256, ef_rows=1, ef_min=33)
        decode("generic kernels")
        assert _lib.ctx_stat(0, 3) == 0  # the generic path does not count its edges: proof that it ran
        ctx_options(tab_cap_e=cap0)
        for pieces in (1, 7):
            ctx_options(pieces=pieces)
            decode(f"pieces={pieces}")
        ctx_options(pieces=0, stage_max_mb=1)
        _lib.trim(0)
        decode("stage_max_mb=1 (overflow, re-run)")
    finally:
        _lib.set_profiling(0, False)
        ctx_options(stage_max_mb=0)
        _lib.trim(0)


# ---- c. plane types and logits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes,P", [("f16", 128), ("bf16", 128), ("bf16", 121), ("logits", 128)])
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_plane_types_and_logits(oracle, mode, A, planes, P):
    """float16 and bfloat16 planes (the oracle is fed the widened values; hw = 121 is no multiple of 8: the narrow load form) and the
    weights as logits (the oracle is fed the device's own softmax): bytes and symbols are the oracle's.  Whether the oracle's decode
    is also round(y) is not asked here - a softmax that sums to a bit above 1 may wrap an edge, in the reference too."""
    for which in ("sweep", "by_channel"):
        x = item(oracle, mode, A, which, True, planes, P)
        assert x.t[1].dtype == {"f16": torch.float16, "bf16": torch.bfloat16, "logits": torch.float32}[planes]
        x.decode("decompress", want_y=False)


# ---- d. mixed launch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_mixed_launch(oracle, ctx_options, mode):
    """2-byte and 4-byte headers, escaped rows and different block sizes in ONE launch, tables landing in 7 pieces with Elias-Fano rows
    from 33 entries on: every item equals its result alone and its oracle answer"""
    y, sg, mu, pi = T.make_latent(501, M=24, h=16, w=12, clamp=False, zero_frac=0.1)
    plain = Item(oracle, mode, f"{mode} make_latent", (y, sg, mu, pi), None, None)
    items = [item(oracle, mode, 125, "sweep"), item(oracle, mode, 126, "sweep"), item(oracle, mode, 125, "nonmono"), plain]
    assert [helpers.hdr_form(x.am + 1) for x in items[:3]] == [2, 4, 2] and plain.am not in (125, 126)
    alone = [x.decode("alone", want_y=(x is not items[2])) for x in items]
    ctx_options(ef_rows=1, ef_min=33, pieces=7)
    res, out = batch(items)
    for x, a, (enc, _), o in zip(items, alone, res, out):
        assert bytes(enc[0]) == bytes(x.compress()[0])
        x.check(o, "mixed launch", want_y=(x is not items[2]))
        assert torch.equal(o, a), x.name


# ---- e. non-monotone item -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_nonmonotone_item(oracle, ctx_options, mode, A):
    """rows that fall: the bytes are the oracle's, and the decoded symbols are oracle.decode_gmm's - NOT y, the reference itself
    desynchronises - on the table path (escaped rows at A = 125, the nonmono bit at A = 126) and on the generic path"""
    x = item(oracle, mode, A, "nonmono")
    assert (x.want_sym != x.sym).any()
    ctx_options(ef_rows=1, ef_min=14)  # every row is long enough for Elias-Fano and must stay raw
    x.decode("table path", want_y=False)
    ctx_options(tab_cap_e=256)
    x.decode("generic path", want_y=False)


# ---- f. segment decoder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_segment_decoder(oracle, ctx_options, mode, A):
    """coded with a note every 256 symbols and decoded by segdec_kernel: the oracle's symbols, the last segment on its own, and
    (settled by the kernel, handed back) == (1, 0) for the monotone items; the non-monotone item is handed back, (0, 1), and the
    table path's answer is the oracle's"""
    ctx_options(gpu_decode=1)
    for which, expect in (("sweep", (1, 0)), ("by_channel", (1, 0)), ("nonmono", (0, 1))):
        x = item(oracle, mode, A, which)
        assert bytes(x.compress(ck=True)[0]) == x.want_bytes
        x.decode("segment decoder", ck=True, want_y=which != "nonmono", last_from=(x.n - 1) // STRIDE * STRIDE)
        assert stat() == expect, f"{x.name}: (settled by the segment decoder, handed back) = {stat()}"


# ---- g. building blocks at other block sizes ------------------------------------------------------------------------------------------
def _first_entry(got, want, max_bs, kinds):
    r, j = (int(a[0]) for a in np.nonzero(got != want))
    return f"row {r} ({kinds[r]}), v = {j - max_bs}: F = {got[r, j]}, the oracle's {want[r, j]}"


@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_building_blocks_at_every_block_size(oracle, ctx_options, mode, A):
    """fgmm_build_tab_hip under the three LDS budgets and fgmm_build_cdftab_hip, on the ladder rows followed by the non-monotone rows:
    the virtual table entry for entry, the reported tl, and the used bytes - the rows', the escape headers' and the padding of every
    block that ends in the middle of a word (tab_kernel places blocks in arrival order: sizes and the virtual table, never raw bytes)"""
    max_bs = A + 1
    sets = [np.concatenate([a, b]) for a, b in zip(W.ladder(mode), W.nonmono_sets())]
    kinds = W.ladder_kinds(mode) + ("nonmono",) * W.P_SETS
    want = oracle.cdftab(mode, *sets, max_bs)  # every sigma is inside the clamp: FGMM_TAB_CLAMP changes nothing but the kernel
    trimmed = W.trim_rows(want)
    saved = helpers.EF_MIN
    try:
        for flags in (0, FGMM_TAB_CLAMP, FGMM_TAB_CLAMP | FGMM_TAB_RAW_ROWS):
            raw = bool(flags & FGMM_TAB_RAW_ROWS)
            helpers.EF_MIN = 1 << 30 if raw else saved  # (expand_trimmed reads the rows as they were built)
            for cap in W.caps(A):
                ctx_options(tab_cap_e=cap)
                h, bo, rows, used, tl = gpu_tab(mode, *sets, max_bs, flags)
                c = W.census(want, max_bs, W.tab_tl(max_bs, cap), None if raw else 14, rows=trimmed)
                assert tl == W.tab_tl(max_bs, cap), (cap, tl)
                got = helpers.expand_trimmed(h, rows, max_bs, bo, tl)
                assert np.array_equal(got, want), f"tab_kernel flags={flags} tl={tl}: {_first_entry(got, want, max_bs, kinds)}"
                assert used == c["used"], (flags, cap, used, c["used"], int(c["bytes"].sum()), c["blocks"].tolist())
            h, p_, used = gpu_cdftab(mode, *sets, max_bs, flags)
            got = helpers.expand_trimmed(h, p_, max_bs)
            assert np.array_equal(got, want), f"cdftab kernels flags={flags}: {_first_entry(got, want, max_bs, kinds)}"
            c = W.census(want, max_bs, W.P_SETS, None if raw else 14, rows=trimmed)
            assert used == int(c["bytes"].sum()) - 4 * int((c["kinds"] == "escaped").sum())  # 4-byte headers: no escape, no padding
    finally:
        helpers.EF_MIN = saved


# ---- h. rate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("A", AS)
@pytest.mark.parametrize("mode", MODES)
def test_rate_of_the_sweep_items(oracle, mode, A):
    """estimate_bits_batch where more than half the symbols are bypass escapes (the integer-cost branch): the relation of
    tests/test_gpu_rate.py - bits_q and n_bypass are the oracle's table priced by the host function, and nbytes is the length of the
    stream compress writes, except where tests/rate_ref.py left_out says it may miss by 4 bytes"""
    L = _lib.lib()
    items = [item(oracle, mode, A, which) for which in ("sweep", "by_channel")]
    est = items[0].gmc.estimate_bits_batch(*([x.t[k] for x in items] for k in range(4)), per_channel=True)
    for x, e in zip(items, est):
        packed = oracle.symtab(mode, x.sym, *x.rows)
        bits_q, nb, cost = R.host_bits(L, packed, x.sym, costs=True)
        assert 4 * nb > x.n, (nb, x.n)
        assert (e.abs_max, e.zero_bitmap.tolist(), e.n_symbols) == (A, x.zb.tolist(), x.n), x.name
        assert (e.bits_q, e.n_bypass) == (bits_q, nb), (x.name, e.bits_q, bits_q, e.n_bypass, nb)
        chan = np.zeros(len(x.zb), np.int64)
        chan[np.nonzero(x.zb)[0]] = cost.reshape(int(x.zb.sum()), -1).astype(np.int64).sum(1)
        bad = np.nonzero(np.asarray(e.channel_bits_q.tolist()) != chan)[0]
        assert bad.size == 0, f"{x.name}: channel {bad[:5]} priced differently"
        assert e.nbytes == L.fgmm_rate_stream_bytes(e.bits_q)
        true_len = len(bytes(x.compress()[0]))
        assert true_len == len(x.want_bytes)
        if R.left_out(R.float_bits(packed, x.sym)):
            assert abs(e.nbytes - true_len) <= 4, (x.name, e.nbytes, true_len)
        else:
            assert e.nbytes == true_len, (x.name, e.nbytes, true_len)
