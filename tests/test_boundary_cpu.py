"""CPU (-m "not gpu"): flashgmm_amd/_boundary.py, the stand-in for the compiled module, against the interface csrc/fgmm_pybind.cpp documents.
No GPU and no context: the addresses are made up, and `_lib.lib()` is a fake that records what each C function is handed - a copy of
the item array - and fills in the outputs a call would.  The expected fields are computed here, from the documentation alone."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

from flashgmm_amd import CheckpointedBytes, _boundary, _lib
from flashgmm_amd.entropy_models import CKPT_DTYPE

NINE = {"compress_stacked", "compress_head_stacked", "decompress_stacked", "compress_items", "decompress_items", "rdoq_stacked", "rdoq_items",
        "rdcurve_items", "rdoq_budget_items"}
CTX, STREAM = 0xC0DE000, 0x57EA000  # a context and a stream: handed through as they are


def test_the_stand_in_has_the_compiled_modules_callables_parameter_for_parameter():
    nat = _lib.native()
    assert nat is not None, "flashgmm_amd/_native*.so missing or not loadable: flashgmm_amd/csrc/build.sh builds it"
    public = {n for n in dir(nat) if not n.startswith("_") and callable(getattr(nat, n))}
    assert public == NINE
    for name in sorted(NINE):
        line = getattr(nat, name).__doc__.splitlines()[0]  # "name(ctx: int, stream: int, ..., bytes_cls: object = None) -> tuple"
        assert line.startswith(name + "(")
        args = line[len(name) + 1:line.rindex(") -> ")]
        want = re.findall(r"(?:^|, )(\w+): ", args)
        defaults = re.findall(r"(\w+): [^,]*? = (\w+)", args)
        sig = inspect.signature(getattr(_boundary, name))
        assert list(sig.parameters) == want, name
        assert [(n, str(p.default)) for n, p in sig.parameters.items() if p.default is not inspect.Parameter.empty] == defaults, name


class FakeLib:
    """records every call as (name, copy of the item array, the other arguments); a compress call returns item i's bitstream
    ``STREAMS[i]`` in a buffer of the fake's and, asked for checkpoints, i notes"""

    def __init__(self, streams=()):
        self.calls, self.streams, self.buffers, self.freed = [], list(streams), [], []

    def fgmm_last_error(self):
        return b""

    def _copy(self, struct, items, n):
        src = items if isinstance(items, C.Array) else C.cast(items, C.POINTER(struct * n)).contents
        assert isinstance(src[0], struct) and len(src) == n
        return (struct * n).from_buffer_copy(src), src

    def _compress(self, name, items, n, rest):
        copy, live = self._copy(_lib.fgmm_item, items, n)
        self.calls.append((name, copy, rest))
        for i, f in enumerate(live):
            buf = C.create_string_buffer(self.streams[i], len(self.streams[i]))
            f.bytes, f.bytes_len, f.abs_max = C.addressof(buf), len(self.streams[i]), 10 + i
            self.buffers.append(buf)
            if f.ckpt_stride and i:
                notes = (_lib.fgmm_ckpt * i)(*[(100 * i + k, 7 * k) for k in range(i)])
                f.ckpt, f.n_ckpt = C.addressof(notes), i
                self.buffers.append(notes)
        return 0

    def fgmm_gmc_compress_batch(self, ctx, stream, items, n, mode, clamp):
        return self._compress("compress", items, n, (ctx, stream, mode, clamp))

    def fgmm_gmc_compress_head_batch(self, ctx, stream, items, xs, n, head, mode, clamp):
        return self._compress("compress_head", items, n, (ctx, stream, list(xs), head, mode, clamp))

    def fgmm_gmc_decompress_batch(self, ctx, stream, items, n, mode, clamp):
        copy, _ = self._copy(_lib.fgmm_item, items, n)
        self.calls.append(("decompress", copy, (ctx, stream, mode, clamp), [C.string_at(f.bytes, f.bytes_len) for f in copy]))
        return 0

    def fgmm_ctx_take_buffers(self, ctx, dst, src, lens, n):
        assert ctx == CTX
        for d, s, l in zip(dst[:n], src[:n], lens[:n]):
            C.memmove(d, s, l)
            self.freed.append(s)
        return 0

    def fgmm_free(self, p):
        self.freed.append(p)

    def fgmm_gmc_rdoq_batch(self, ctx, stream, items, n, mode, clamp, lam):
        copy, live = self._copy(_lib.fgmm_rdoq_item, items, n)
        self.calls.append(("rdoq", copy, (ctx, stream, mode, clamp, lam)))
        for i, f in enumerate(live):
            f.n_changed, f.bits_q_before, f.bits_q_after, f.abs_max = i, (1 << 40) + i, (1 << 39) + i, 3 + i
        return 0

    def fgmm_gmc_rdoq_batch_s(self, ctx, stream, items, n, mode, clamp, lam, weights, skip):
        self.calls.append(("rdoq_s", self._copy(_lib.fgmm_rdoq_item, items, n)[0], (ctx, stream, mode, clamp, lam), weights, skip))
        return 0

    def fgmm_gmc_rdcurve_batch_s(self, ctx, stream, items, n, mode, clamp, lambdas, n_lambdas, weights, skip):
        self.calls.append(("rdcurve_s", self._copy(_lib.fgmm_rdcurve_item, items, n)[0], (ctx, stream, mode, clamp, list(lambdas[:n_lambdas])), weights, skip))
        return 0

    def fgmm_gmc_rdoq_budget_batch_s(self, ctx, stream, items, n, mode, clamp, groups, n_groups, budgets, lambda_max, refine, res, weights, skip):
        self.calls.append(("budget_s", self._copy(_lib.fgmm_rdoq_item, items, n)[0],
                           (ctx, stream, mode, clamp, None if groups is None else list(groups[:n]), n_groups, list(budgets[:n_groups]), lambda_max, refine),
                           weights, skip))
        for g in range(n_groups):
            res[g].lambda_, res[g].bytes_pred, res[g].passes, res[g].status = 0.5 * g, 1000 + g, 3, 7 * (g & 1)
        return 0


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: f)
    return f


# made-up addresses, far enough apart that a wrong stride or element size lands on another value
Y, S, MU, W, YQ, ZB, X, HEAD, CHAN = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000, 0x60000000, 0x70000000, 0x7F000000, 0x68000000
N, M, HW, K = 3, 5, 12, 4
STREAMS = [b"\x01\x02\x03\x04", b"", bytes(range(200)) * 2]


def check_inputs(f, i, item_stride, esz, dtype, flags, with_y=True):
    """the input fields of stacked item i: planes at base + i * item_stride elements of esz bytes, y dense float32"""
    off = i * item_stride * esz
    assert (f.params.scales, f.params.means, f.params.weights) == (S + off, MU + off, W + off)
    assert (f.params.stride_k, f.params.stride_c, f.params.dtype, f.params.flags) == (M * HW, HW, dtype, flags)
    assert (f.M, f.K, f.hw) == (M, K, HW) and f.y == (Y + i * M * HW * 4 if with_y else None)


@pytest.mark.parametrize("dtype,esz", [(_lib.FGMM_F32, 4), (_lib.FGMM_F16, 2), (_lib.FGMM_BF16, 2)])
@pytest.mark.parametrize("stride_factor", [1, 2])
@pytest.mark.parametrize("ckpt_stride", [0, 256])
def test_compress_stacked_items_and_results(fake, dtype, esz, stride_factor, ckpt_stride):
    fake.streams = STREAMS
    item_stride = stride_factor * K * M * HW
    cls = CheckpointedBytes if ckpt_stride else None
    strings, amax = _boundary.compress_stacked(CTX, STREAM, Y, S, MU, W, N, M, HW, item_stride, M * HW, HW, dtype, 1, 2, 1, ckpt_stride, YQ, ZB, cls)
    (name, items, rest), = fake.calls
    assert name == "compress" and rest == (CTX, STREAM, 2, 1) and len(items) == N
    for i, f in enumerate(items):
        check_inputs(f, i, item_stride, esz, dtype, 1)
        assert f.yq_out == YQ + i * M * HW * 4 and f.zero_bitmap == ZB + i * M * 8 and f.ckpt_stride == ckpt_stride
        assert not f.bytes and not f.ckpt and f.n_ckpt == 0 and f.bytes_len == 0
    assert amax == [10, 11, 12] and [bytes(s) for s in strings] == STREAMS and all(type(s) is (cls or bytes) for s in strings)
    assert len(fake.freed) == (5 if ckpt_stride else 3)  # every library buffer handed back: three bitstreams, two arrays of notes
    if ckpt_stride:
        for i, s in enumerate(strings):
            blob, first, count, addr, stride = s._ck
            assert isinstance(blob, bytes) and len(blob) == 16 * 3 and (first, count, stride) == ((0, 0, 1)[i], i, ckpt_stride)
            assert s.ckpt.dtype == CKPT_DTYPE and s.ckpt.tolist() == [(100 * i + k, 7 * k) for k in range(i)] and s.ckpt_stride == ckpt_stride
            assert (addr == 0) if not i else C.string_at(addr, 16 * i) == s.ckpt.tobytes()


def test_a_large_batch_of_plain_bitstreams_is_copied_by_the_library(fake):
    """from 256 KiB on, plain bytes objects are allocated at their size and filled by fgmm_ctx_take_buffers (one call)"""
    fake.streams = [bytes([i]) * (100000 + i) for i in range(N)]
    strings, _ = _boundary.compress_stacked(CTX, STREAM, Y, S, MU, W, N, M, HW, K * M * HW, M * HW, HW, 0, 0, 0, 1, 0, YQ, ZB)
    assert strings == fake.streams and all(type(s) is bytes for s in strings) and len(fake.freed) == N


def test_compress_head_stacked_has_no_planes_and_one_feature_pointer_per_item(fake):
    fake.streams = STREAMS
    c_in = 9
    strings, amax = _boundary.compress_head_stacked(CTX, STREAM, Y, X, HEAD, N, M, c_in, HW, 1, 0, 0, YQ, ZB)
    (name, items, rest), = fake.calls
    assert name == "compress_head" and rest == (CTX, STREAM, [X + i * c_in * HW * 4 for i in range(N)], HEAD, 1, 0)
    for i, f in enumerate(items):
        assert (f.params.scales, f.params.means, f.params.weights) == (None, None, None)
        assert (f.params.dtype, f.params.flags) == (_lib.FGMM_F32, _lib.FGMM_PARAMS_LOGITS) and (f.M, f.K, f.hw) == (M, K, HW)
        assert (f.y, f.yq_out, f.zero_bitmap, f.ckpt_stride) == (Y + i * M * HW * 4, YQ + i * M * HW * 4, ZB + i * M * 8, 0)
    assert strings == STREAMS and amax == [10, 11, 12]


def checkpointed_streams():
    """plain bytes, a CheckpointedBytes whose ``_ck`` holds an ndarray (as its constructor makes it) and one whose ``_ck`` names
    records 2 .. 5 of a blob (as a compress call attaches it) -> the streams and per stream (ckpt, n_ckpt, ckpt_stride)"""
    notes = np.zeros(2, CKPT_DTYPE)
    notes["x"], notes["pos"] = [1 << 40, 1 << 41], [5, 9]
    a = CheckpointedBytes(b"second stream", notes, 512)
    blob = np.arange(2 * 6, dtype="<u8").tobytes()
    b = CheckpointedBytes(b"third", np.zeros(0, CKPT_DTYPE), 0)
    b._ck = (blob, 2, 3, 0xABC000 + 32, 1024)
    return [b"first", a, b], [(None, 0, 0), (a.ckpt.ctypes.data, 2, 512), (0xABC000 + 32, 3, 1024)], (notes, blob)


@pytest.mark.parametrize("dtype,esz", [(_lib.FGMM_F32, 4), (_lib.FGMM_BF16, 2)])
@pytest.mark.parametrize("stride_factor", [1, 2])
def test_decompress_stacked_items(fake, dtype, esz, stride_factor):
    strings, cks, alive = checkpointed_streams()
    item_stride, zb_row = stride_factor * K * M * HW, 2 * M  # (every second row of a larger batch's bitmaps)
    got = _boundary.decompress_stacked(CTX, STREAM, strings, [4, 5, 6], ZB, zb_row, S, MU, W, N, M, HW, item_stride, M * HW, HW, dtype, 1, 0, 1, YQ,
                                       CheckpointedBytes)
    (name, items, rest, seen), = fake.calls
    assert got is None and name == "decompress" and rest == (CTX, STREAM, 0, 1) and seen == [bytes(s) for s in strings]
    for i, f in enumerate(items):
        check_inputs(f, i, item_stride, esz, dtype, 1, with_y=False)
        assert f.yq_out == YQ + i * M * HW * 4 and f.zero_bitmap == ZB + i * zb_row * 8 and f.abs_max == 4 + i
        assert f.bytes_len == len(strings[i]) and (f.ckpt, f.n_ckpt, f.ckpt_stride) == cks[i]
    # without the class nobody's notes are read; something that is not bytes is refused before the call
    _boundary.decompress_stacked(CTX, STREAM, strings, [4, 5, 6], ZB, M, S, MU, W, N, M, HW, item_stride, M * HW, HW, dtype, 0, 0, 1, YQ)
    assert all((f.ckpt, f.n_ckpt, f.ckpt_stride) == (None, 0, 0) for f in fake.calls[1][1])
    with pytest.raises(RuntimeError, match="bitstream 1 is not a bytes object"):
        _boundary.decompress_stacked(CTX, STREAM, [b"", bytearray(b"x"), b""], [4, 5, 6], ZB, M, S, MU, W, N, M, HW, item_stride, M * HW, HW, dtype, 0, 0, 1, YQ)
    assert len(fake.calls) == 2


# the sequence form: items of three shapes, each with planes of its own type
SEQ = [(0x1000 * (i + 1), 0x2000 * (i + 1), 0x3000 * (i + 1), m, hw, m * sc, sc, 0x5000 * (i + 1), 0x6000 * (i + 1), dt)
       for i, (m, hw, sc, dt) in enumerate([(5, 12, 12, _lib.FGMM_F32), (8, 6, 7, _lib.FGMM_BF16), (1, 1, 1, _lib.FGMM_F16)])]


def check_sequence_item(f, t, flags):
    s, mu, w, m, hw, sk, sc, out, zb, dt = t
    assert (f.params.scales, f.params.means, f.params.weights, f.params.stride_k, f.params.stride_c) == (s, mu, w, sk, sc)
    assert (f.params.dtype, f.params.flags, f.M, f.K, f.hw, f.yq_out, f.zero_bitmap) == (dt, flags, m, K, hw, out, zb)


@pytest.mark.parametrize("ckpt_stride", [0, 256])
def test_compress_items_carry_their_own_dtype(fake, ckpt_stride):
    fake.streams = STREAMS
    tuples = [(0x900 * (i + 1),) + t for i, t in enumerate(SEQ)]
    strings, amax = _boundary.compress_items(CTX, STREAM, tuples, 1, 2, 0, ckpt_stride, CheckpointedBytes if ckpt_stride else None)
    (name, items, rest), = fake.calls
    assert name == "compress" and rest == (CTX, STREAM, 2, 0) and len(items) == 3
    for i, f in enumerate(items):
        check_sequence_item(f, SEQ[i], 1)
        assert f.y == 0x900 * (i + 1) and f.ckpt_stride == ckpt_stride and not f.bytes and not f.ckpt
    assert [bytes(s) for s in strings] == STREAMS and amax == [10, 11, 12]
    assert [len(s.ckpt) for s in strings] == [0, 1, 2] if ckpt_stride else all(type(s) is bytes for s in strings)
    with pytest.raises(RuntimeError, match="an item is"):
        _boundary.compress_items(CTX, STREAM, [t[:-1] for t in tuples], 1, 2, 0, 0)


def test_decompress_items_carry_their_own_dtype(fake):
    strings, cks, alive = checkpointed_streams()
    _boundary.decompress_items(CTX, STREAM, strings, [7, 8, 9], SEQ, 0, 1, 1, CheckpointedBytes)
    (name, items, rest, seen), = fake.calls
    assert name == "decompress" and rest == (CTX, STREAM, 1, 1) and seen == [bytes(s) for s in strings]
    for i, f in enumerate(items):
        check_sequence_item(f, SEQ[i], 0)
        assert f.y is None and f.abs_max == 7 + i and f.bytes_len == len(strings[i]) and (f.ckpt, f.n_ckpt, f.ckpt_stride) == cks[i]
    with pytest.raises(RuntimeError, match="3 items, 2 bitstreams"):
        _boundary.decompress_items(CTX, STREAM, strings[:2], [7, 8], SEQ, 0, 1, 1)


@pytest.mark.parametrize("chan_after", [0, CHAN])
@pytest.mark.parametrize("dtype,esz,stride_factor", [(_lib.FGMM_F32, 4, 1), (_lib.FGMM_F16, 2, 2)])
def test_rdoq_stacked_items_and_results(fake, dtype, esz, stride_factor, chan_after):
    item_stride = stride_factor * K * M * HW
    got = _boundary.rdoq_stacked(CTX, STREAM, Y, S, MU, W, N, M, HW, item_stride, M * HW, HW, dtype, 0, 1, 1, 0.25, YQ, ZB, chan_after)
    (name, items, rest), = fake.calls
    assert name == "rdoq" and rest == (CTX, STREAM, 1, 1, 0.25)
    for i, f in enumerate(items):
        check_inputs(f, i, item_stride, esz, dtype, 0)
        assert f.y_rdo == YQ + i * M * HW * 4 and f.zero_bitmap == ZB + i * M * 8
        assert f.chan_bits_q_after == (chan_after + i * M * 8 if chan_after else None)
    assert got == ([0, 1, 2], [(1 << 40) + i for i in range(N)], [(1 << 39) + i for i in range(N)], [3, 4, 5])


def test_the_calls_that_take_their_items_by_address(fake):
    """rdoq_items, rdcurve_items, rdoq_budget_items: the caller's arrays reach the library as they are; lambdas, groups and budgets
    as C arrays; weights and skip null unless given"""
    rd, cv = (_lib.fgmm_rdoq_item * 2)(), (_lib.fgmm_rdcurve_item * 2)()
    wts, sk, csk = (_lib.fgmm_rdo_weights * 2)(), (_lib.fgmm_rdo_skip * 2)(), (_lib.fgmm_rdcurve_skip * 2)()
    rd[1].M, cv[1].M, wts[1].chan_w, sk[1].skipped = 33, 44, 0x123000, 0x456000
    same = lambda p, arr: C.addressof(p.contents) == C.addressof(arr)  # noqa: E731
    _boundary.rdoq_items(CTX, STREAM, C.addressof(rd), 2, 0, 1, 0.5)
    _boundary.rdoq_items(CTX, STREAM, C.addressof(rd), 2, 0, 1, 0.5, C.addressof(wts), C.addressof(sk))
    (n0, i0, r0, w0, s0), (n1, i1, r1, w1, s1) = fake.calls
    assert n0 == n1 == "rdoq_s" and r0 == r1 == (CTX, STREAM, 0, 1, 0.5) and i0[1].M == i1[1].M == 33
    assert w0 is None and s0 is None and same(w1, wts) and same(s1, sk) and w1[1].chan_w == 0x123000 and s1[1].skipped == 0x456000
    lambdas = [0.0, 0.125, 3.5] + [float(i) for i in range(13)]
    _boundary.rdcurve_items(CTX, STREAM, C.addressof(cv), 2, 2, 0, lambdas, 0, C.addressof(csk))
    name, items, rest, w, s = fake.calls[2]
    assert name == "rdcurve_s" and rest == (CTX, STREAM, 2, 0, lambdas) and items[1].M == 44 and w is None and same(s, csk)
    res = _boundary.rdoq_budget_items(CTX, STREAM, C.addressof(rd), 2, 0, 1, [1, 0], [5000, 1 << 40], 16.0, 2, C.addressof(wts))
    name, items, rest, w, s = fake.calls[3]
    assert name == "budget_s" and rest == (CTX, STREAM, 0, 1, [1, 0], 2, [5000, 1 << 40], 16.0, 2) and same(w, wts) and s is None
    assert res == [(0.0, 1000, 3, 0), (0.5, 1001, 3, 7)]
    _boundary.rdoq_budget_items(CTX, STREAM, C.addressof(rd), 2, 0, 1, None, [7, 8], 4.0, 0)
    assert fake.calls[4][2] == (CTX, STREAM, 0, 1, None, 2, [7, 8], 4.0, 0)


def test_a_status_is_raised_with_the_calls_name(fake, monkeypatch):
    monkeypatch.setattr(fake, "fgmm_gmc_decompress_batch", lambda *a: 1)
    monkeypatch.setattr(fake, "fgmm_last_error", lambda: b"item 1: dtype")
    with pytest.raises(_lib.FgmmError, match="GaussianMixtureConditional.decompress: FGMM_ERR_INVALID: item 1: dtype"):
        _boundary.decompress_items(CTX, STREAM, [b"a", b"b", b"c"], [1, 2, 3], SEQ, 0, 0, 1)


def test_boundary_follows_native_at_every_call(monkeypatch):
    """_lib.boundary(): the compiled module while _lib.native() gives one - looked up at call time, however it is turned off"""
    nat = _lib.native()
    assert nat is not None and _lib.boundary() is nat
    with monkeypatch.context() as m:
        m.setattr(_lib, "_native", False)
        assert _lib.native() is None and _lib.boundary() is _boundary
    with monkeypatch.context() as m:
        m.setattr(_lib, "native", lambda: None)
        assert _lib.boundary() is _boundary
    proxy = object()
    with monkeypatch.context() as m:
        m.setattr(_lib, "native", lambda: proxy)
        assert _lib.boundary() is proxy
    assert _lib.boundary() is nat
