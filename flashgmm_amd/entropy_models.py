"""``GaussianMixtureConditional`` — the Python boundary of the path, same API as the reference's class
(compressai/entropy_models/entropy_models.py:762-910), running on MI355X.

    gmc = GaussianMixtureConditional(K=4)
    (strings, abs_max, zero_bitmap), y_q = gmc.compress(y, scales, means, weights)
    y_hat = gmc.decompress(strings, abs_max, zero_bitmap, scales, means, weights)

``y`` is ``[1, M, h, w]``; ``scales / means / weights`` are ``[1, K*M, h, w]`` with channel ``k*M + c``
(latent_codecs/gaussian_mixture_conditional.py:193-202).  What the reference does on the host between these
tensors and its C++ coder — abs-max, round, zero-channel bitmap, channel gather, the (n,K) re-layout with the
sigma clamp, four ``.to("cpu")`` copies — is fused into the HIP kernels: parameters are read in place from the
planar layout and only the 4 B/symbol table crosses PCIe.  Returned values and bitstreams are identical to the
reference's for identical inputs.

Intended deviation: ``decompress`` returns ``y_hat`` on the parameters' device (the reference builds it on the
CPU, entropy_models.py:905-908, and lets the caller's assignment copy it back).
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import Tensor

from . import _boundary, _lib

__all__ = ["GaussianMixtureConditional", "EntropyBottleneck", "EntropyBottleneckCoder", "CheckpointedBytes", "CompressedBatch", "ParameterHead", "RateEstimate", "RdoQuantized", "RdoSkipQuantized", "BudgetQuantized", "RdCurve", "update_entropy_models", "aux_loss"]

CKPT_DTYPE = np.dtype([("x", "<u8"), ("pos", "<u8")])  # fgmm_ckpt

class CheckpointedBytes(bytes):
    """A bitstream — the reference's, byte for byte: it IS a ``bytes`` object and compares equal to one — that also carries
    its encoder's out-of-band CHECKPOINTS (``include/flashgmm_amd.h``: ``fgmm_ckpt``): the coder state and the stream
    position before every ``stride``-th symbol.  ``GaussianMixtureConditional.decompress`` decodes the segments between them
    on all host workers instead of one (every segment is verified against the next checkpoint; wrong ones cost a
    sequential decode, never a wrong symbol).  Anything that only knows ``bytes`` — the reference's decoder, a file — sees
    the plain stream; ``flashgmm_amd.container`` stores the checkpoints next to it."""

    # _ck = (notes, first, count, address, stride): `notes` is an ndarray of CKPT_DTYPE (first = 0), or the ``bytes`` blob a compress
    # call filled with the notes of ALL its bitstreams (adopt_ckpts of either binding sets the record on an instance whose bytes are
    # already in place) - this one's are records first .. first + count of it, the view is made when someone asks for ``.ckpt``;
    # address: of the first note (what a decode call reads off the record and hands the library)
    def __new__(cls, data: bytes, ckpt: np.ndarray, stride: int):
        self = super().__new__(cls, data)
        if not (isinstance(ckpt, np.ndarray) and ckpt.dtype == CKPT_DTYPE and ckpt.flags.c_contiguous):
            ckpt = np.ascontiguousarray(ckpt, dtype=CKPT_DTYPE)
        self._ck = (ckpt, 0, len(ckpt), ckpt.ctypes.data if len(ckpt) else 0, int(stride))  # (ndarray.ctypes is slow: taken once)
        return self

    @property
    def ckpt(self) -> np.ndarray:
        """[(x: u64, pos: u64)], entry k = before symbol (k + 1) * stride"""
        notes, first, count, addr, stride = self._ck
        if not isinstance(notes, np.ndarray):
            notes = np.frombuffer(notes, dtype=CKPT_DTYPE, count=count, offset=16 * first) if count else _NO_CKPT
            self._ck = (notes, 0, count, addr, stride)
        return notes

    @property
    def ckpt_stride(self) -> int:
        return self._ck[4]

    @property
    def _ckpt_addr(self) -> int:
        return self._ck[3]

    def __reduce__(self):
        return (CheckpointedBytes, (bytes(self), self.ckpt, self.ckpt_stride))


_NO_CKPT = np.zeros(0, CKPT_DTYPE)


class CompressedBatch(Sequence):
    """What ``compress_batch`` returns for STACKED inputs: the N results held as the call produced them - ``strings`` (list of
    N ``bytes``), ``abs_maxes`` (list of N ints), ``zero_bitmaps`` (one ``[N, M]`` int64 CPU tensor), ``y_q`` (one
    ``[N, 1, M, h, w]`` tensor).  It IS the sequence of ``((bytes, abs_max, zero_bitmap), y_q)`` the list form returns -
    ``len``, indexing, slicing and iteration give the per-item tuples (views, made when asked for) - and its fields go
    straight back into ``decompress_batch`` (``strings[s::2]``, ``zero_bitmaps[s::2]`` ...) without 2 N tensor views
    being built for a caller that never looks at them."""

    __slots__ = ("strings", "abs_maxes", "zero_bitmaps", "y_q")

    def __init__(self, strings: List[bytes], abs_maxes: List[int], zero_bitmaps: Tensor, y_q: Tensor):
        self.strings, self.abs_maxes, self.zero_bitmaps, self.y_q = strings, abs_maxes, zero_bitmaps, y_q

    def __len__(self) -> int:
        return len(self.strings)

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self.strings)))]
        return (self.strings[i], self.abs_maxes[i], self.zero_bitmaps[i]), self.y_q[i]

    # list semantics where they are cheap (callers written against the list a sequence-input call returns): concatenation
    # gives a plain list of the per-item tuples
    def __add__(self, other):
        return list(self) + list(other)

    def __radd__(self, other):
        return list(other) + list(self)


class RateEstimate:
    """The coded size of one latent, computed on the GPU WITHOUT running the coder (``GaussianMixtureConditional.estimate_bits`` /
    ``estimate_bits_batch``; include/flashgmm_amd.h section 3b):

    ``bits_q``       exact ideal code length of the symbols ``compress`` would code, in units of 2^-24 bit (an integer: the same
                     on every run);  ``bits`` = ``bits_q / 2**24``
    ``nbytes``       predicted ``len(bytes)`` of the bitstream: ``4 * ((bits_q + (64 << 24)) >> 29)`` - the stream's length, except
                     where ``bits`` lies within the coder's accumulated rounding of a multiple of 32 (then 4 bytes off)
    ``n_symbols``    symbols coded (coded channels x h x w);  ``n_bypass``: those that take the bypass escape
    ``abs_max``, ``zero_bitmap``   what ``compress`` returns (``zero_bitmap``: int64 ``[M]`` CPU tensor)
    ``channel_bits_q`` / ``channel_bits``   per channel, int64 / float64 ``[M]`` CPU tensors (``per_channel=True``; else None)
    ``latent_bits``  float32 ``[1, M, h, w]`` on the inputs' device: bits per latent, 0 in the channels that are not coded
                     (``per_latent=True``; else None)"""

    __slots__ = ("bits_q", "nbytes", "n_symbols", "n_bypass", "abs_max", "zero_bitmap", "channel_bits_q", "latent_bits")

    def __init__(self, bits_q, nbytes, n_symbols, n_bypass, abs_max, zero_bitmap, channel_bits_q=None, latent_bits=None):
        self.bits_q, self.nbytes, self.n_symbols, self.n_bypass = int(bits_q), int(nbytes), int(n_symbols), int(n_bypass)
        self.abs_max, self.zero_bitmap, self.channel_bits_q, self.latent_bits = int(abs_max), zero_bitmap, channel_bits_q, latent_bits

    @property
    def bits(self) -> float:
        return self.bits_q / float(1 << _lib.FGMM_RATE_Q)

    @property
    def channel_bits(self):
        return None if self.channel_bits_q is None else self.channel_bits_q.to(torch.float64) / float(1 << _lib.FGMM_RATE_Q)

    def __repr__(self) -> str:
        return f"RateEstimate(bits={self.bits:.3f}, nbytes={self.nbytes}, n_symbols={self.n_symbols}, n_bypass={self.n_bypass}, abs_max={self.abs_max})"


class RdoQuantized:
    """A latent quantised with rate-distortion optimisation (``GaussianMixtureConditional.quantize_rdo`` / ``quantize_rdo_batch``;
    include/flashgmm_amd.h section 3c): per latent of a coded channel ``round(y)`` or one of its two neighbours, whichever minimises
    ``(y - v)**2 + lam * bits(v)`` under the coder's own exact cost.

    ``y``            float32 ``[1, M, h, w]`` on the inputs' device, integer-valued: ``compress(result.y, ...)`` codes it unchanged
    ``n_changed``    latents whose symbol is not ``round(y)``
    ``bits_q_before`` / ``bits_q_after``   exact cost of ``round(y)`` / of the chosen symbols over the channels coded for the input, in
                     units of 2^-24 bit (integers: the same on every run);  ``bits_before`` / ``bits_after`` in bits
    ``abs_max``, ``zero_bitmap``   what ``compress(result.y, ...)`` returns (``zero_bitmap``: int64 ``[M]`` CPU tensor)
    ``channel_bits_q_after``   per channel, int64 ``[M]`` CPU tensor (``per_channel=True``; else None)"""

    __slots__ = ("y", "n_changed", "bits_q_before", "bits_q_after", "abs_max", "zero_bitmap", "channel_bits_q_after")

    def __init__(self, y, n_changed, bits_q_before, bits_q_after, abs_max, zero_bitmap, channel_bits_q_after=None):
        self.y, self.n_changed, self.bits_q_before, self.bits_q_after = y, int(n_changed), int(bits_q_before), int(bits_q_after)
        self.abs_max, self.zero_bitmap, self.channel_bits_q_after = int(abs_max), zero_bitmap, channel_bits_q_after

    @property
    def bits_before(self) -> float:
        return self.bits_q_before / float(1 << _lib.FGMM_RATE_Q)

    @property
    def bits_after(self) -> float:
        return self.bits_q_after / float(1 << _lib.FGMM_RATE_Q)

    def __repr__(self) -> str:
        return f"RdoQuantized(n_changed={self.n_changed}, bits_before={self.bits_before:.3f}, bits_after={self.bits_after:.3f}, abs_max={self.abs_max})"


# what a budget search adds to an RdoQuantized: None on the result of quantize_rdo (the slots of RdoQuantized itself stay what they are)
RdoQuantized.lam = RdoQuantized.bytes_pred = RdoQuantized.budget_met = RdoQuantized.passes = None
# what channel skipping adds (section 3f): None where it was not asked for
RdoQuantized.n_skipped = RdoQuantized.n_eligible = RdoQuantized.skipped = RdoQuantized.ddist_q = None


class RdoSkipQuantized(RdoQuantized):
    """The ``RdoQuantized`` of a call with ``channel_skip=True`` (include/flashgmm_amd.h section 3f): after the per-latent decisions,
    a coded channel is dropped whole - its plane of ``y`` zero, nothing of it in the stream - where that lowers distortion + lam * bits.
    The inherited sums are those after the channel decisions; ``estimate_bits(result.y, ...)`` returns exactly ``bits_q_after``.

    ``n_skipped``    channels skipped;  ``n_eligible``  coded channels that may be (every latent finite, ``|round(y)| <= 15``)
    ``skipped``      bool ``[M]`` CPU tensor (``per_channel=True``; else None)
    ``ddist_q``      the (weighted) squared error ``y`` adds over ``round(input)``, units of 2^-32"""

    __slots__ = ("n_skipped", "n_eligible", "skipped", "ddist_q")

    def __init__(self, y, n_changed, bits_q_before, bits_q_after, abs_max, zero_bitmap, channel_bits_q_after=None, skip=None):
        super().__init__(y, n_changed, bits_q_before, bits_q_after, abs_max, zero_bitmap, channel_bits_q_after)
        self.n_skipped, self.n_eligible, self.skipped, self.ddist_q = skip if skip is not None else (None, None, None, None)


class BudgetQuantized(RdoSkipQuantized):
    """The ``RdoQuantized`` of a latent quantised to a byte budget (``GaussianMixtureConditional.quantize_to_budget`` /
    ``quantize_to_budget_batch``; include/flashgmm_amd.h section 3d), with what the search found for the latent's GROUP:

    ``lam``          the lambda found - every other field is ``quantize_rdo``'s at this lambda, bit for bit
    ``bytes_pred``   predicted bytes of the group's bitstreams at ``lam`` (the sum over its items)
    ``budget_met``   False: no lambda up to ``lambda_max`` meets the budget; the result is the one at ``lambda_max``
    ``passes``       passes of the curve kernel the group took part in

    The budget is on predicted bytes: a real stream may be 4 bytes longer where ``RateEstimate.nbytes`` may be; a channel the
    quantisation empties is no longer coded at all, so on that account the real size can only be smaller - unless the search ran
    with ``channel_skip=True``, where such a channel counts nothing (``n_skipped``, ``n_eligible``, ``skipped``, ``ddist_q``: as
    ``RdoSkipQuantized``'s; None otherwise)."""

    __slots__ = ("lam", "bytes_pred", "budget_met", "passes")

    def __init__(self, y, n_changed, bits_q_before, bits_q_after, abs_max, zero_bitmap, channel_bits_q_after=None, lam=None, bytes_pred=None,
                 budget_met=None, passes=None, skip=None):
        super().__init__(y, n_changed, bits_q_before, bits_q_after, abs_max, zero_bitmap, channel_bits_q_after, skip)
        self.lam, self.bytes_pred, self.budget_met, self.passes = lam, bytes_pred, budget_met, passes

    def __repr__(self) -> str:
        return (f"BudgetQuantized(lam={self.lam!r}, bytes_pred={self.bytes_pred}, budget_met={self.budget_met}, passes={self.passes}, "
                f"n_changed={self.n_changed}, bits_after={self.bits_after:.3f})")


class RdCurve:
    """A stretch of the rate-distortion curve of one latent (``GaussianMixtureConditional.rd_curve`` / ``rd_curve_batch``;
    include/flashgmm_amd.h section 3d): what ``quantize_rdo`` would report at each of ``lambdas``, from one pass per 16 of them.

    ``lambdas``        the lambdas, as given (any order, repeats allowed)
    ``bits_q_before``  exact cost of ``round(y)``, units of 2^-24 bit
    ``bits_q_after``   per lambda: exact cost of the chosen symbols;  ``bits_after`` in bits, ``nbytes`` the predicted stream length
    ``n_changed``      per lambda: latents whose symbol is not ``round(y)``
    ``ddist_q``        per lambda: squared error the moves add over ``round(y)``, units of 2^-32;  ``distortion_added`` as floats.
                       WEIGHTED - each latent's share times ``channel_weights[c] * position_weights[p]`` - when the call was given
                       weights (section 3e)
    ``n_symbols``      symbols coded (coded channels x h x w)
    ``n_skipped``      per lambda: channels skipped (``channel_skip=True``, section 3f - the three sums above are then those after the
                       channel decisions); None otherwise
    ``n_eligible``     coded channels that may be skipped, as ``RdoSkipQuantized.n_eligible`` (``channel_skip=True``; else None)"""

    __slots__ = ("lambdas", "bits_q_before", "bits_q_after", "n_changed", "ddist_q", "n_symbols", "n_skipped", "n_eligible")

    def __init__(self, lambdas, bits_q_before, bits_q_after, n_changed, ddist_q, n_symbols=0, n_skipped=None, n_eligible=None):
        self.n_skipped = None if n_skipped is None else tuple(map(int, n_skipped))
        self.n_eligible = None if n_eligible is None else int(n_eligible)
        self.lambdas, self.bits_q_before = tuple(float(v) for v in lambdas), int(bits_q_before)
        self.bits_q_after, self.n_changed, self.ddist_q = tuple(map(int, bits_q_after)), tuple(map(int, n_changed)), tuple(map(int, ddist_q))
        self.n_symbols = int(n_symbols)

    @property
    def bits_after(self):
        return tuple(b / float(1 << _lib.FGMM_RATE_Q) for b in self.bits_q_after)

    @property
    def nbytes(self):
        f = _lib.lib().fgmm_rate_stream_bytes
        return tuple(int(f(b)) for b in self.bits_q_after)

    @property
    def distortion_added(self):
        return tuple(d / float(1 << 32) for d in self.ddist_q)

    def __repr__(self) -> str:
        return f"RdCurve(lambdas={self.lambdas}, nbytes={self.nbytes}, n_changed={self.n_changed})"


def _ctx_stream(dev: torch.device) -> Tuple[int, int]:
    """-> (address of the device's context, the caller's current stream): what every native call begins with"""
    return _lib.ctx_addr(dev.index if dev.index is not None else -1), torch.cuda.current_stream(dev).cuda_stream


class _LatentItems:
    """The items of one call that prices latents, built by ``GaussianMixtureConditional._latent_items`` from either input form:
    ``arr`` the ``struct[N]`` ctypes passes, ``items`` the same memory as a numpy record array (filled and read column by column),
    ``keep`` the input tensors whose storage the items name; for the outputs' shapes ``shape``, the ``(1, M, h, w)`` of every item
    of a stacked batch, or ``ys``, the latents of a sequence."""

    DTYPES = {_lib.fgmm_rate_item: _lib.RATE_ITEM_DTYPE, _lib.fgmm_rdoq_item: _lib.RDOQ_ITEM_DTYPE, _lib.fgmm_rdcurve_item: _lib.RDCURVE_ITEM_DTYPE,
              _lib.fgmm_like_item: _lib.LIKE_ITEM_DTYPE, _lib.fgmm_like_grad_item: _lib.LIKE_GRAD_ITEM_DTYPE,
              _lib.fgmm_centroid_item: _lib.CENTROID_ITEM_DTYPE}
    __slots__ = ("arr", "items", "N", "keep", "dev", "shape", "ys")

    def __init__(self, struct, N, keep, dev=None, shape=None, ys=None):
        self.arr = (struct * N)()
        self.items, self.N = np.frombuffer(self.arr, self.DTYPES[struct]), N
        self.keep, self.dev, self.shape, self.ys = keep, dev, shape, ys

    def call(self) -> Tuple[int, int]:
        return _ctx_stream(self.dev)

    def output(self, field: str, dtype, per_latent: bool = False):
        """allocates the output ``field`` of every item - per latent ``[1, M, h, w]`` on the device, else per channel ``[M]`` on the
        host; ONE ``[N, ...]`` tensor for stacked input, one per item for sequences - and writes the addresses -> the items' tensors
        (the caller holds them across the call)"""
        device = self.dev if per_latent else None
        if self.shape is not None:
            t = torch.empty((self.N,) + (self.shape if per_latent else self.shape[1:2]), dtype=dtype, device=device)
            self.items[field] = np.uint64(t.data_ptr()) + np.arange(self.N, dtype=np.uint64) * np.uint64(t.stride(0) * t.element_size())
            return t.unbind(0)
        ts = [torch.empty((1, M) + tuple(y.shape[2:]) if per_latent else (M,), dtype=dtype, device=device)
              for M, y in zip(self.items["M"].tolist(), self.ys)]
        self.items[field] = [t.data_ptr() for t in ts]
        return ts


def _rdo_weight_lists(ys, channel_weights, position_weights):
    """THE validation of the factors of a weighted call (include/flashgmm_amd.h section 3e), before anything native runs -> None (no
    factors at all), or per item ``(chan_w or None, pos_w or None)``: contiguous float32 tensors ``[M]`` / ``[h * w]`` on the
    latents' device.  ``channel_weights``: one ``[M]`` tensor for the batch, or a sequence of one (or None) per item;
    ``position_weights``: per item ``[h, w]`` or ``[1, 1, h, w]`` (or None), ``[N, 1, h, w]`` for stacked latents.  The factors'
    VALUES (finite, 0 .. 256) are checked on the device by the call itself."""
    if channel_weights is None and position_weights is None:
        return None
    stacked = isinstance(ys, Tensor)
    N = ys.shape[0] if stacked else len(ys)
    lat = [ys[i:i + 1] for i in range(N)] if stacked else list(ys)

    def one(t, what, i, shapes):
        if t is None:
            return None
        if not isinstance(t, Tensor):
            raise TypeError(f"{what}[{i}]: a float32 tensor or None, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"{what}[{i}]: must be float32, got {t.dtype}")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{what}[{i}]: shape {tuple(t.shape)}, expected {' or '.join(str(s) for s in shapes)}")
        if t.device != lat[i].device:
            raise ValueError(f"{what}[{i}]: on {t.device}, the latents are on {lat[i].device}")
        return t.contiguous().view(-1)

    def per_item(arg, what, shared_ok):
        if arg is None:
            return [None] * N
        if isinstance(arg, Tensor):
            if shared_ok:
                return [arg] * N
            if stacked:
                if arg.dim() != 4 or arg.shape[0] != N:
                    raise ValueError(f"{what}: shape {tuple(arg.shape)}, expected [{N}, 1, h, w] for stacked latents")
                return [arg[i:i + 1] for i in range(N)]
            raise ValueError(f"{what}: a sequence of one tensor (or None) per item for a sequence of latents")
        arg = list(arg)
        if len(arg) != N:
            raise ValueError(f"{what}: one per item ({N}), got {len(arg)}")
        return arg

    cws = per_item(channel_weights, "channel_weights", True)
    pws = per_item(position_weights, "position_weights", False)
    out = []
    for i, y in enumerate(lat):
        if y.dim() != 4:
            raise ValueError(f"latent {i}: expected 4 dimensions, got {tuple(y.shape)}")
        M, h, w = y.shape[1:]
        out.append((one(cws[i], "channel_weights", i, [(M,)]), one(pws[i], "position_weights", i, [(h, w), (1, 1, h, w)])))
    return out


def _one_item(t):
    """the single calls' ``position_weights`` as the batch calls take it"""
    return None if t is None else [t]


def _rdo_weights_array(lists):
    """per item ``(chan_w, pos_w)`` tensors -> the ``fgmm_rdo_weights[N]`` ctypes passes (None: no factors, the unweighted call)"""
    if lists is None or all(c is None and p is None for c, p in lists):
        return None
    arr = (_lib.fgmm_rdo_weights * len(lists))()
    for a, (c, p) in zip(arr, lists):
        a.chan_w, a.pos_w = (c.data_ptr() if c is not None else None), (p.data_ptr() if p is not None else None)
    return arr


def _rdo_skip_array(L, per_channel):
    """the ``fgmm_rdo_skip[N]`` of a call with channel skipping (section 3f) and, ``per_channel``, the items' host int64 ``[M]`` flags"""
    arr = (_lib.fgmm_rdo_skip * L.N)()
    flags = [None] * L.N
    if per_channel:
        flags = [torch.empty((int(M),), dtype=torch.int64) for M in L.items["M"].tolist()]
        for a, t in zip(arr, flags):
            a.skipped = t.data_ptr()
    return arr, flags


def _rdo_skip_cols(arr, flags):
    """-> per item ``(n_skipped, n_eligible, skipped bool [M] or None, ddist_q)``"""
    return [(int(a.n_skipped), int(a.n_eligible), None if t is None else t != 0, int(a.ddist_q)) for a, t in zip(arr, flags)]


def _addr(arr) -> int:
    """the address of an optional ctypes array as the boundary takes it (None: 0)"""
    return C.addressof(arr) if arr is not None else 0


def _plane_view(t: Tensor, K: int) -> Tuple[Tensor, int, int]:
    """-> (tensor kept alive, stride_k, stride_c) for a [1, K*M, h, w] parameter tensor whose (h, w) planes are
    dense; anything else is made contiguous first.  chunk(3, 1) views of the parameter head qualify as they are."""
    shape = t.shape
    if len(shape) != 4 or shape[0] != 1:
        raise RuntimeError("entropy parameters must be [1, K*M, h, w] (the reference squeezes batch 1 too, entropy_models.py:841)")
    if t.dtype not in _PARAM_DTYPES:
        raise RuntimeError(f"entropy parameters must be float32, float16 or bfloat16, got {t.dtype}")
    hw = shape[2] * shape[3]
    st = t.stride()
    if hw > 1 and not (st[3] == 1 and st[2] == shape[3]):
        t = t.contiguous()
        st = t.stride()
    sc = st[1] if shape[1] > 1 else hw
    return t, (shape[1] // K) * sc, sc


_PARAM_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_ABI_DTYPE = {torch.float32: _lib.FGMM_F32, torch.float16: _lib.FGMM_F16, torch.bfloat16: _lib.FGMM_BF16}


def _abi_dtype(dt: torch.dtype) -> int:
    """the fgmm_dtype of parameter planes of torch dtype `dt` (include/flashgmm_amd.h section 2)"""
    try:
        return _ABI_DTYPE[dt]
    except KeyError:
        raise RuntimeError(f"entropy parameters must be float32, float16 or bfloat16, got {dt}") from None


class ParameterHead:
    """The last layer of the reference's ``entropy_parameters`` - ``nn.Conv2d(c_in, 3*K*M, 1)`` (compressai/models/ckbd_gmm.py:115-121) -
    with the ``chunk(3, 1)`` / softmax-over-K that follows it (latent_codecs/gaussian_mixture_conditional.py:183-202), on the matrix
    cores in ONE fixed summation order (include/flashgmm_amd.h section 2b: bit for bit an ``fmaf`` chain over the input channels):

        head = ParameterHead(entropy_parameters[-1])                       # any nn.Conv2d(c_in, 3*K*M, 1) on the GPU
        scales, means, logits = head.params(x)                             # x [N, c_in, h, w] -> three [N, K*M, h, w] views
        res = gmc.compress_head_batch(y, x, head)                          # the same parameters, never written to HBM
        y_hat = gmc.decompress_batch(res.strings, res.abs_maxes, res.zero_bitmaps, scales, means, logits, weights_are_logits=True)

    Encoder and decoder then derive identical parameters from identical weights whatever BLAS / MIOpen version either side
    runs - the reference relies on that silently.  The weights are packed once, here.

    ``arithmetic="bf16x6"`` is within ``R (sum_k |w x| + |b|) + 2^-133 sum_k (|w_k| + |x_k|) + 6 n16 2^-150`` of the exact result,
    ``n16 = ceil(c_in / 16)``, ``R = 2^-23 (1 + 2^-6) + 6 n16 2^-24 (1 + 2^-7)``, on its domain: finite operands below 0x1.FFp127.
    Weights outside it raise here; an item whose features leave it is computed by the exact form (the fmaf chain, bit for bit)."""

    def __init__(self, conv, K: int = 4, arithmetic: str = "f32"):
        # arithmetic: "f32" (the default: binary32 products and sums on v_mfma_f32_32x32x2_f32, bit for bit an fmaf chain) or "bf16x6"
        # (three bfloat16 parts per operand, six part products on the BF16 matrix cores, binary32 accuracy at a third of the cycles;
        # deterministic on MI355X, not restatable on a CPU: include/flashgmm_amd.h FGMM_HEAD_BF16X6)
        if arithmetic not in ("f32", "bf16x6"):
            raise ValueError(f"arithmetic {arithmetic!r}")
        self.arithmetic = arithmetic
        w = conv.weight.detach()
        if w.dim() != 4 or w.shape[2:] != (1, 1) or w.shape[0] % (3 * K) or not w.is_cuda:
            raise RuntimeError("expected the weights of a 1x1 nn.Conv2d(c_in, 3*K*M) on a HIP device")
        self.K, self.M, self.c_in = int(K), int(w.shape[0] // (3 * K)), int(w.shape[1])
        self.device = w.device
        self._dev = w.device.index if w.device.index is not None else -1
        w2 = w.reshape(w.shape[0], w.shape[1]).to(torch.float32).contiguous()
        b = None if conv.bias is None else conv.bias.detach().to(torch.float32).contiguous()
        out = C.c_void_p()
        stream = torch.cuda.current_stream(w.device).cuda_stream
        _lib.check(_lib.lib().fgmm_head_create_ex(_lib.ctx(self._dev), stream, w2.data_ptr(), b.data_ptr() if b is not None else None, self.M, self.K,
                                                  self.c_in, _lib.FGMM_HEAD_BF16X6 if arithmetic == "bf16x6" else 0, C.byref(out)), "ParameterHead")
        self._h = out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().fgmm_head_destroy(h)
            except Exception:  # pragma: no cover - interpreter shutdown
                pass

    def _features(self, x: Tensor) -> Tensor:
        if x.dim() != 4 or x.shape[1] != self.c_in or x.device != self.device:
            raise RuntimeError(f"features must be [N, {self.c_in}, h, w] on {self.device}; got {tuple(x.shape)} on {x.device}")
        return x.to(torch.float32).contiguous()

    def params(self, x: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        """-> (scales, means, logits): views ``[N, K*M, h, w]`` of one ``[N, 3*K*M, h, w]`` tensor - what ``entropy_parameters[-1](x)
        .chunk(3, 1)`` gives, in the library's summation order.  ``logits``: pass ``weights_are_logits=True`` to the coder."""
        x = self._features(x)
        N, _, h, w = x.shape
        out = torch.empty((N, 3 * self.K * self.M, h, w), dtype=torch.float32, device=x.device)
        if N and h * w:
            per_x, per_o = self.c_in * h * w * 4, 3 * self.K * self.M * h * w * 4
            xs = (C.c_void_p * N)(*[x.data_ptr() + i * per_x for i in range(N)])
            os_ = (C.c_void_p * N)(*[out.data_ptr() + i * per_o for i in range(N)])
            hws = (C.c_int64 * N)(*([h * w] * N))
            _lib.check(_lib.lib().fgmm_head_params_batch(_lib.ctx(self._dev), torch.cuda.current_stream(x.device).cuda_stream, self._h, xs, os_, hws, N),
                       "ParameterHead.params")
        return tuple(out.chunk(3, 1))


def _like_forward(gmc, x, scales, means, weights, rnd: bool, want_map: bool, logits: bool):
    """the forward call of section 3g, or 3h (``logits``) -> ``(main, v, n_nonfinite)`` as ``_LikelihoodFn`` returns them"""
    L = gmc._latent_items(_lib.fgmm_like_item, x, scales, means, weights, logits)
    if L.N == 0:
        raise RuntimeError("the likelihood needs a batch of at least one item")
    N, (_, M, h, w), dev = L.N, L.shape, L.dev
    step = np.arange(N, dtype=np.uint64) * np.uint64(M * h * w * 4)
    like = v = None
    if want_map:
        like = torch.empty((N, M, h, w), dtype=torch.float32, device=dev)
        L.items["like_out"] = np.uint64(like.data_ptr()) + step
    if rnd:
        v = torch.empty((N, M, h, w), dtype=torch.float32, device=dev)
        L.items["v_out"] = np.uint64(v.data_ptr()) + step
    call = _lib.lib().fgmm_gmc_likelihood_logits_batch if logits else _lib.lib().fgmm_gmc_likelihood_batch
    rc = call(*L.call(), L.arr, N, int(rnd), gmc.scale_bound, gmc.likelihood_bound)
    _lib.check(rc, "GaussianMixtureConditional.forward")
    nonfinite = torch.from_numpy(L.items["n_nonfinite"].astype(np.int64))
    main = like if want_map else torch.from_numpy(L.items["bits_q"].astype(np.float64) * 2.0 ** -_lib.FGMM_LIKE_Q).to(dev)
    return main, v, nonfinite


def _like_backward(gmc, x, scales, means, weights, rnd: bool, want_map: bool, logits: bool, g_main, need_x: bool, planes):
    """the backward call of section 3g, or 3h (``logits``) -> dy ``[N, M, h, w]`` float32 (``need_x``; else None).  ``planes``: None,
    or per item the byte addresses ``(dscales, dmeans, dweights)`` as three uint64 arrays ``[N]`` - the caller's float32 ``[K, M, h, w]``
    blocks the twelve gradient planes of an item are written to"""
    L = gmc._latent_items(_lib.fgmm_like_grad_item, x, scales, means, weights, logits)
    N, (_, M, h, w), dev = L.N, L.shape, L.dev
    rng = np.arange(N, dtype=np.uint64)
    dy = None
    if need_x:
        dy = torch.empty((N, M, h, w), dtype=torch.float32, device=dev)
        L.items["dy"] = np.uint64(dy.data_ptr()) + rng * np.uint64(M * h * w * 4)
    if planes is not None:
        L.items["dscales"], L.items["dmeans"], L.items["dweights"] = planes
    if want_map:
        g = g_main.to(torch.float32).contiguous()  # (held until the call returns: the call waits for its kernel)
        L.items["g_like"] = np.uint64(g.data_ptr()) + rng * np.uint64(M * h * w * 4)
    else:
        L.items["g_bits"] = g_main.detach().to("cpu", torch.float64).numpy()
    call = _lib.lib().fgmm_gmc_likelihood_logits_backward_batch if logits else _lib.lib().fgmm_gmc_likelihood_backward_batch
    rc = call(*L.call(), L.arr, N, int(rnd), gmc.scale_bound, gmc.likelihood_bound)
    _lib.check(rc, "GaussianMixtureConditional.forward (backward)")
    return dy


class _LikelihoodFn(torch.autograd.Function):
    """``GaussianMixtureConditional.forward`` / ``rate_bits`` on the GPU (include/flashgmm_amd.h section 3g): one kernel forward, one
    backward that recomputes everything from the inputs - nothing but the inputs is saved.  ``x`` ``[B, M, h, w]`` float32 is the
    latent (``rnd``: rounded by the kernel) or the already-noised values.  -> ``(main, v, n_nonfinite)``: ``main`` the likelihood map
    ``[B, M, h, w]`` (``want_map``) or the items' bits as float64 ``[B]``; ``v`` the rounded latent (``rnd``; else None);
    ``n_nonfinite`` int64 ``[B]`` on the CPU, the latents left out of the bits.  ``logits``: section 3h - ``weights`` holds the
    parameter head's logits, the softmax over K and its derivative run in the kernels, and the gradient returned in the ``weights``
    slot is the logits'."""

    @staticmethod
    def forward(ctx, gmc, x, scales, means, weights, rnd: bool, want_map: bool, logits: bool):
        main, v, nonfinite = _like_forward(gmc, x, scales, means, weights, rnd, want_map, logits)
        ctx.save_for_backward(x, scales, means, weights)
        ctx.gmc, ctx.rnd, ctx.want_map, ctx.logits = gmc, rnd, want_map, logits
        ctx.mark_non_differentiable(nonfinite)
        if v is not None:
            ctx.mark_non_differentiable(v)
        return main, v, nonfinite

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_main, g_v, g_nonfinite):
        x, scales, means, weights = ctx.saved_tensors
        gmc, rnd = ctx.gmc, ctx.rnd
        need_x, need_s, need_m, need_w = ctx.needs_input_grad[1:5]
        need_x = need_x and not rnd  # round() has gradient zero: None
        if g_main is None or not (need_x or need_s or need_m or need_w):
            return (None,) * 8
        N, KM, h, w = scales.shape
        rng = np.arange(N, dtype=np.uint64) * np.uint64(KM * h * w * 4)

        def out(need):
            if not need:
                return None, np.zeros(N, np.uint64)
            t = torch.empty((N, KM, h, w), dtype=torch.float32, device=scales.device)
            return t, np.uint64(t.data_ptr()) + rng

        (ds, ps), (dm, pm), (dw, pw) = out(need_s), out(need_m), out(need_w)
        dy = _like_backward(gmc, x, scales, means, weights, rnd, ctx.want_map, ctx.logits, g_main, need_x, (ps, pm, pw))
        cast = lambda t, like: None if t is None else t.to(like.dtype)  # noqa: E731
        return None, dy, cast(ds, scales), cast(dm, means), cast(dw, weights), None, None, None


class _LikelihoodParamsFn(torch.autograd.Function):
    """``GaussianMixtureConditional.forward_params`` / ``rate_bits_params`` (section 3h): ``_LikelihoodFn`` with ``logits`` on the three
    thirds of the parameter head's output ``params`` ``[B, 3*K*M, h, w]`` (scales | means | logits), passed as the strided views they
    are.  The backward writes the thirty-six gradient planes of an item straight into ONE ``[B, 3*K*M, h, w]`` float32 tensor, the
    gradient of ``params``: no ``chunk`` backward runs, nothing is concatenated."""

    @staticmethod
    def forward(ctx, gmc, x, params, rnd: bool, want_map: bool):
        main, v, nonfinite = _like_forward(gmc, x, *params.chunk(3, 1), rnd, want_map, True)
        ctx.save_for_backward(x, params)
        ctx.gmc, ctx.rnd, ctx.want_map = gmc, rnd, want_map
        ctx.mark_non_differentiable(nonfinite)
        if v is not None:
            ctx.mark_non_differentiable(v)
        return main, v, nonfinite

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_main, g_v, g_nonfinite):
        x, params = ctx.saved_tensors
        need_x, need_p = ctx.needs_input_grad[1:3]
        need_x = need_x and not ctx.rnd
        if g_main is None or not (need_x or need_p):
            return (None,) * 5
        dp = planes = None
        if need_p:
            N, KM3, h, w = params.shape
            dp = torch.empty((N, KM3, h, w), dtype=torch.float32, device=params.device)
            third = (KM3 // 3) * h * w * 4
            base = np.uint64(dp.data_ptr()) + np.arange(N, dtype=np.uint64) * np.uint64(3 * third)
            planes = (base, base + np.uint64(third), base + np.uint64(2 * third))
        dy = _like_backward(ctx.gmc, x, *params.chunk(3, 1), ctx.rnd, ctx.want_map, True, g_main, need_x, planes)
        return None, dy, (None if dp is None else dp.to(params.dtype)), None, None


class GaussianMixtureConditional(nn.Module):
    """Entropy model of a K-component Gaussian mixture conditional; ``compress`` / ``decompress`` only need K = 4
    (the reference's coder is bound for K = 4 only, rans_interface.cpp:60,982).  Calling the module (``forward``) gives the
    differentiable likelihoods evaluation and training use, ``rate_bits`` their fused rate (section 3g)."""

    def __init__(self, K: int = 4, mode=None, clamp_scales: bool = True, checkpoint_stride: int = 0, scale_bound: float = 0.11,
                 likelihood_bound: float = 1e-9):
        super().__init__()
        # forward()'s two LowerBounds, the reference's defaults (entropy_models.py:113, 636); compress / decompress do not use them
        self.scale_bound, self.likelihood_bound = float(scale_bound), float(likelihood_bound)
        if not 0.0 < self.scale_bound < float("inf"):
            raise ValueError("Invalid parameters")  # (entropy_models.py:656-657)
        if not 0.0 <= self.likelihood_bound < float("inf"):
            raise ValueError("likelihood_bound must be finite and >= 0 (0: no bound)")
        self.K = int(K)
        self.mode = mode  # None -> APPROX_MODE env var at call time
        self.clamp_scales = bool(clamp_scales)  # entropy_models.py:817 clamp(0.11, 256)
        # > 0: compress() returns CheckpointedBytes (the same bytes + out-of-band checkpoints every that many symbols, a power
        # of two >= 256), which decompress() decodes on all host workers; 0 (the default): plain bytes, as the reference's
        self.checkpoint_stride = int(checkpoint_stride)
        if self.checkpoint_stride and (self.checkpoint_stride < 256 or self.checkpoint_stride & (self.checkpoint_stride - 1)):
            raise ValueError("checkpoint_stride must be 0 or a power of two >= 256")

    # ------------------------------------------------------------------------------------------------
    def _mode(self) -> int:
        return _lib.default_mode() if self.mode is None else _lib.mode_id(self.mode)

    def reshape_entropy_parameters(self, scales, means, weights, nonzero):
        """Same result as the reference (entropy_models.py:810-828): three (n, K) views with strides (1, n), sigma
        clamped.  The HIP path never materialises these; kept for callers and tests that want the coder inputs."""
        reshape_size = (scales.size(0), self.K, scales.size(1) // self.K, -1)

        def rs(t):
            return t.reshape(*reshape_size)[:, :, nonzero].permute(1, 0, 2, 3).reshape(self.K, -1).permute(1, 0)

        return rs(scales).clamp(0.11, 256), rs(means), rs(weights)

    # ------------------------------------------------------------------------------------------------
    def _check_k(self):
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the kernels are bound for K = 4 only (as the reference's coder)")

    def likelihood(self, values: Tensor, scales: Tensor, means: Tensor, weights: Tensor, *, round: bool = False,
                   weights_are_logits: bool = False) -> Tuple[Tensor, Tensor]:
        """The building block of ``forward``: -> ``(v, likelihood)`` with ``v = torch.round(values)`` (``round=True``) or ``values``
        itself, and the bounded mixture likelihood of ``v`` (include/flashgmm_amd.h section 3g).  Differentiable in ``scales``,
        ``means``, ``weights`` and, without rounding, ``values``.  ``weights_are_logits`` (section 3h): ``weights`` holds the parameter
        head's logits, the softmax over K runs in the kernel - the coder's own sequence - and the gradient ``weights`` receives is the
        logits'."""
        self._check_k()
        like, v, _ = _LikelihoodFn.apply(self, values, scales, means, weights, bool(round), True, bool(weights_are_logits))
        return (v if round else values), like

    def forward(self, inputs: Tensor, scales: Tensor, means: Tensor, weights: Tensor, training: Optional[bool] = None, *,
                weights_are_logits: bool = False) -> Tuple[Tensor, Tensor]:
        """As the reference's (entropy_models.py:792-808): -> ``(outputs, likelihood)``.  ``inputs`` ``[B, M, h, w]`` float32,
        ``scales / means / weights`` ``[B, K*M, h, w]`` float32, float16 or bfloat16, ``weights`` the mixture weights themselves (the
        softmax over K stays torch's, so autograd differentiates it).  ``training`` (default ``self.training``): ``outputs`` is
        ``inputs`` plus uniform noise in [-0.5, 0.5) drawn by torch; otherwise ``torch.round(inputs)``.  One fused HIP kernel
        evaluates the likelihood, one recomputes it for the gradients (returned in the inputs' dtypes); in evaluation mode ``inputs``
        receives no gradient, as through ``torch.round``.  ``weights_are_logits``: as in ``likelihood``."""
        self._check_k()
        if training is None:
            training = self.training
        if training:
            outputs = inputs + torch.empty_like(inputs).uniform_(-0.5, 0.5)  # quantize(inputs, "noise") (entropy_models.py:163-167)
            return self.likelihood(outputs, scales, means, weights, weights_are_logits=weights_are_logits)
        return self.likelihood(inputs, scales, means, weights, round=True, weights_are_logits=weights_are_logits)

    def rate_bits(self, inputs: Tensor, scales: Tensor, means: Tensor, weights: Tensor, training: Optional[bool] = None, *,
                  return_nonfinite: bool = False, weights_are_logits: bool = False):
        """The fused rate of ``forward``: -> ``(outputs, bits)``, ``bits`` a float64 tensor ``[B]`` on the inputs' device - per item
        ``sum(-log2(likelihood))``, summed on the GPU as integers in units of 2^-32 bit (the same bits on every run), differentiable
        like the sum it stands for.  No likelihood map is written or kept.  Latents whose likelihood is NaN, infinite or <= 0 are left
        out of the sum; ``return_nonfinite=True`` adds their count as a third value, an int64 ``[B]`` CPU tensor.
        ``weights_are_logits``: as in ``likelihood``."""
        self._check_k()
        if training is None:
            training = self.training
        outputs = inputs + torch.empty_like(inputs).uniform_(-0.5, 0.5) if training else inputs
        bits, v, nonfinite = _LikelihoodFn.apply(self, outputs, scales, means, weights, not training, False, bool(weights_are_logits))
        outputs = outputs if training else v
        return (outputs, bits, nonfinite) if return_nonfinite else (outputs, bits)

    def _check_params(self, params: Tensor):
        if params.dim() != 4 or params.size(1) % (3 * self.K):
            raise RuntimeError(f"params must be [B, 3*K*M, h, w], scales | means | logits; got {tuple(params.shape)}")

    def forward_params(self, inputs: Tensor, params: Tensor, training: Optional[bool] = None) -> Tuple[Tensor, Tensor]:
        """``forward`` on the parameter head's output as it is (section 3h): ``params`` ``[B, 3*K*M, h, w]`` float32, float16 or
        bfloat16, ordered scales | means | logits as ``chunk(3, 1)`` splits it.  The softmax over K and its derivative run in the two
        kernels, on the three thirds in place; the backward writes ONE float32 ``[B, 3*K*M, h, w]`` tensor, the gradient of ``params``
        (cast to its dtype where that is not float32) - no softmax, ``chunk`` or concatenation runs in torch on either pass.
        -> ``(outputs, likelihood)``, bit for bit those of ``forward(inputs, *params.chunk(3, 1), weights_are_logits=True)``."""
        self._check_k()
        self._check_params(params)
        if training is None:
            training = self.training
        outputs = inputs + torch.empty_like(inputs).uniform_(-0.5, 0.5) if training else inputs
        like, v, _ = _LikelihoodParamsFn.apply(self, outputs, params, not training, True)
        return (outputs if training else v), like

    def rate_bits_params(self, inputs: Tensor, params: Tensor, training: Optional[bool] = None, *, return_nonfinite: bool = False):
        """``rate_bits`` on the parameter head's output as it is: ``params`` and the gradient it receives as in ``forward_params``."""
        self._check_k()
        self._check_params(params)
        if training is None:
            training = self.training
        outputs = inputs + torch.empty_like(inputs).uniform_(-0.5, 0.5) if training else inputs
        bits, v, nonfinite = _LikelihoodParamsFn.apply(self, outputs, params, not training, False)
        outputs = outputs if training else v
        return (outputs, bits, nonfinite) if return_nonfinite else (outputs, bits)

    # ------------------------------------------------------------------------------------------------
    def _item_ints(self, y: Optional[Tensor], scales: Tensor, means: Tensor, weights: Tensor, keep: list):
        """THE validation of one item of the sequence form -> (pointers and strides as integers, M, hw, device, fgmm_dtype of the planes);
        the tensors whose storage the pointers name are appended to ``keep``"""
        if not scales.is_cuda:
            raise RuntimeError(
                "flashgmm_amd runs the GMM entropy-coding path on the GPU only: tensors must be on a HIP device "
                "(there is deliberately no CPU fallback)")
        s, sk, sc = _plane_view(scales, self.K)
        m, mk, mc = _plane_view(means, self.K)
        w, wk, wc = _plane_view(weights, self.K)
        if (mk, mc) != (sk, sc) or (wk, wc) != (sk, sc) or m.shape != s.shape or w.shape != s.shape:
            if m.shape != s.shape or w.shape != s.shape:
                raise RuntimeError("scales, means and weights must have one shape")
            s, m, w = s.contiguous(), m.contiguous(), w.contiguous()
            hw_ = s.size(2) * s.size(3)
            sc, sk = hw_, (s.size(1) // self.K) * hw_
        if not (s.dtype == m.dtype == w.dtype):
            raise RuntimeError("scales, means and weights must share one dtype")
        shp = s.shape
        M = shp[1] // self.K
        hw = shp[2] * shp[3]
        keep += [s, m, w]
        yp = 0
        if y is not None:
            ys_ = y.shape
            if len(ys_) != 4 or ys_[0] != 1 or ys_[1] != M or ys_[2] * ys_[3] != hw:
                raise RuntimeError(f"y must be [1, {M}, h, w] matching the parameters; got {tuple(ys_)}")
            if y.dtype != torch.float32 or y.device != s.device:  # latents stay float32 (32 B/symbol with fp16 planes)
                raise RuntimeError("y must be float32 on the parameters' device")
            yc = y.contiguous()
            yp = yc.data_ptr()
            keep.append(yc)
        return yp, s.data_ptr(), m.data_ptr(), w.data_ptr(), M, hw, sk, sc, s.device, _abi_dtype(s.dtype)

    def _stacked_view(self, y: Optional[Tensor], scales: Tensor, means: Tensor, weights: Tensor):
        """THE validation of stacked inputs -> (y, scales, means, weights, N, M, h, w, item stride, stride_c)"""
        if not scales.is_cuda:
            raise RuntimeError(
                "flashgmm_amd runs the GMM entropy-coding path on the GPU only: tensors must be on a HIP device "
                "(there is deliberately no CPU fallback)")
        if scales.dim() != 4 or means.shape != scales.shape or weights.shape != scales.shape:
            raise RuntimeError("stacked entropy parameters must be three [N, K*M, h, w] tensors of one shape")
        if not (scales.dtype == means.dtype == weights.dtype) or scales.dtype not in _PARAM_DTYPES:
            raise RuntimeError("scales, means and weights must share one dtype, float32, float16 or bfloat16")
        N, KM, h, w = scales.shape
        st = scales.stride()
        if (h * w > 1 and not (st[3] == 1 and st[2] == w)) or means.stride() != st or weights.stride() != st:
            scales, means, weights = scales.contiguous(), means.contiguous(), weights.contiguous()
            st = scales.stride()
        M = KM // self.K
        if y is not None:
            if y.dim() != 4 or tuple(y.shape) != (N, M, h, w):
                raise RuntimeError(f"y must be [{N}, {M}, {h}, {w}] matching the parameters; got {tuple(y.shape)}")
            if y.dtype != torch.float32 or y.device != scales.device:
                raise RuntimeError("y must be float32 on the parameters' device")
            y = y.contiguous()
        return y, scales, means, weights, N, M, h, w, st[0], (st[1] if KM > 1 else h * w)

    def _compress_stacked(self, y: Tensor, scales: Tensor, means: Tensor, weights: Tensor, flags: int = 0):
        y, scales, means, weights, N, M, h, w, s_item, sc = self._stacked_view(y, scales, means, weights)
        dev = scales.device
        yq = torch.empty((N, 1, M, h, w), dtype=torch.float32, device=dev)
        zb = torch.empty((N, M), dtype=torch.int64)
        if N == 0:
            return CompressedBatch([], [], zb, yq)
        strings, amax = _lib.boundary().compress_stacked(
            *_ctx_stream(dev), y.data_ptr(), scales.data_ptr(), means.data_ptr(), weights.data_ptr(),
            N, M, h * w, s_item, M * sc, sc, _abi_dtype(scales.dtype), flags, self._mode(),
            int(self.clamp_scales), self.checkpoint_stride, yq.data_ptr(), zb.data_ptr(), CheckpointedBytes if self.checkpoint_stride else None)
        return CompressedBatch(strings, amax, zb, yq)

    def _decompress_stacked(self, strings: Sequence[bytes], abs_maxes: Sequence[int], zero_bitmaps, scales: Tensor,
                            means: Tensor, weights: Tensor, flags: int = 0, stacked_output: bool = False):
        _, scales, means, weights, N, M, h, w, s_item, sc = self._stacked_view(None, scales, means, weights)
        if len(strings) != N or len(abs_maxes) != N or len(zero_bitmaps) != N:
            raise RuntimeError(f"{N} items in the parameter tensors, {len(strings)} bitstreams")
        dev = scales.device
        y_hat = torch.empty((N, 1, M, h, w), dtype=torch.float32, device=dev)
        if N > 0:
            zb = zero_bitmaps if isinstance(zero_bitmaps, Tensor) else torch.stack([z.to("cpu", torch.int64) for z in zero_bitmaps])
            if zb.device.type != "cpu" or zb.dtype != torch.int64:
                zb = zb.to("cpu", torch.int64)
            if tuple(zb.shape) != (N, M):
                raise RuntimeError(f"zero bitmaps have shape {tuple(zb.shape)}, expected ({N}, {M})")
            if M > 1 and zb.stride(1) != 1:
                zb = zb.contiguous()
            if not isinstance(strings, list) or not all(type(s_) is bytes or isinstance(s_, bytes) for s_ in strings):
                strings = [s_ if isinstance(s_, bytes) else bytes(s_) for s_ in strings]
            # (zb's rows may be a strided view of a larger batch - a codec stage: every second one; the out-of-band notes of the
            # bitstreams that carry them are read off the objects)
            _lib.boundary().decompress_stacked(*_ctx_stream(dev), strings, abs_maxes,
                                               zb.data_ptr(), zb.stride(0) if N > 1 else M, scales.data_ptr(), means.data_ptr(), weights.data_ptr(), N, M, h * w, s_item,
                                               M * sc, sc, _abi_dtype(scales.dtype), flags, self._mode(), int(self.clamp_scales),
                                               y_hat.data_ptr(), CheckpointedBytes)
        return y_hat if stacked_output else list(y_hat.unbind(0))

    def compress_batch(self, ys, scales, means, weights, *, weights_are_logits: bool = False):
        """N independent ``compress`` calls in one native call (kernels batched over items, one host rANS worker
        per bitstream).  Returns a sequence of ``((bytes, abs_max, zero_bitmap_cpu), y_q)`` - a list, or for stacked inputs a
        ``CompressedBatch`` (the same sequence, held stacked).

        The items are given either as sequences of ``[1, M, h, w]`` / ``[1, K*M, h, w]`` tensors (any mix of shapes)
        or, for items of one shape, stacked: ``y [N, M, h, w]``, parameters ``[N, K*M, h, w]`` — what a network
        evaluated on a batch of images produces, and the cheaper form (one check, one allocation per output).

        ``weights_are_logits``: ``weights`` holds the parameter head's logits and the softmax over K
        (latent_codecs/gaussian_mixture_conditional.py:198-202) runs inside the HIP kernels — the pi plane is never written
        and read back.  ``decompress`` must then be given the logits too."""
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        flags = _lib.FGMM_PARAMS_LOGITS if weights_are_logits else 0
        if isinstance(ys, Tensor):
            return self._compress_stacked(ys, scales, means, weights, flags)
        n_items = len(ys)
        if n_items == 0:
            return []
        keep, tuples, outs, ms, dev = [], [], [], [], None  # the items as tuples of integers (fgmm_pybind.cpp: compress_items)
        for i in range(n_items):
            yp, sp, mp, wp, M, hw, sk, sc, d, dt = self._item_ints(ys[i], scales[i], means[i], weights[i], keep)
            dev = dev or d
            if d != dev:
                raise RuntimeError("all items of a batch must be on one device")
            yq = torch.empty_like(keep[-1])
            outs.append(yq)
            ms.append(M)
            tuples.append([yp, sp, mp, wp, M, hw, sk, sc, yq.data_ptr(), 0, dt])
        zb_all = torch.empty(sum(ms), dtype=torch.int64)  # the zero bitmaps of all items: one allocation, a view per item
        at, base = 0, zb_all.data_ptr()
        for t, M in zip(tuples, ms):
            t[9] = base + 8 * at
            at += M
        strings, amax = _lib.boundary().compress_items(*_ctx_stream(dev), [tuple(t) for t in tuples], flags, self._mode(), int(self.clamp_scales),
                                                       self.checkpoint_stride, CheckpointedBytes if self.checkpoint_stride else None)
        bitmaps = zb_all.split(ms)
        return [((strings[i], amax[i], bitmaps[i]), outs[i].view_as(ys[i])) for i in range(n_items)]

    def compress_head_batch(self, y: Tensor, x: Tensor, head: "ParameterHead") -> CompressedBatch:
        """``compress_batch`` with the parameter head FUSED into the encode-side CDF kernel: ``y [N, M, h, w]`` latents, ``x [N, c_in, h, w]``
        the features the head's last convolution reads.  The 3*K parameters of a latent go from the matrix cores' accumulators into
        its table entry; the parameter tensors are never written.  The bitstreams are those of
        ``compress_batch(y, *head.params(x), weights_are_logits=True)``, byte for byte."""
        if self.K != _lib.FGMM_K or head.K != self.K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        x = head._features(x)
        N, _, h, w = x.shape
        M = head.M
        if y.dim() != 4 or tuple(y.shape) != (N, M, h, w) or y.dtype != torch.float32 or y.device != x.device:
            raise RuntimeError(f"y must be float32 [{N}, {M}, {h}, {w}] on the features' device; got {tuple(y.shape)}")
        dev = x.device
        if N == 0:
            return CompressedBatch([], [], torch.empty((0, M), dtype=torch.int64), torch.empty((0, 1, M, h, w), dtype=torch.float32, device=dev))
        y = y.contiguous()
        yq = torch.empty((N, 1, M, h, w), dtype=torch.float32, device=dev)
        zb = torch.empty((N, M), dtype=torch.int64)
        strings, amax = _lib.boundary().compress_head_stacked(
            *_ctx_stream(dev), y.data_ptr(), x.data_ptr(), head._h.value,
            N, M, head.c_in, h * w, self._mode(), int(self.clamp_scales), self.checkpoint_stride, yq.data_ptr(), zb.data_ptr(),
            CheckpointedBytes if self.checkpoint_stride else None)
        return CompressedBatch(strings, amax, zb, yq)

    def estimate_bits_batch(self, ys, scales, means, weights, *, weights_are_logits: bool = False, per_channel: bool = False,
                            per_latent: bool = False) -> List[RateEstimate]:
        """The size of what ``compress_batch`` would return for the same arguments, WITHOUT coding: one kernel does the encode-side
        CDF kernel's arithmetic and sums the exact code length (no table, nothing but a few KB across PCIe, no host coder).
        Inputs as ``compress_batch`` takes them - sequences of ``[1, M, h, w]`` / ``[1, K*M, h, w]`` tensors, or stacked.
        -> one ``RateEstimate`` per item; ``per_channel`` / ``per_latent`` add the per-channel sums and the per-latent map."""
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        L = self._latent_items(_lib.fgmm_rate_item, ys, scales, means, weights, weights_are_logits)
        if L.N == 0:
            return []
        bitmaps = L.output("zero_bitmap", torch.int64)
        chans = L.output("chan_bits_q", torch.int64) if per_channel else [None] * L.N
        maps = L.output("bits_map", torch.float32, per_latent=True) if per_latent else [None] * L.N
        rc = _lib.lib().fgmm_gmc_estimate_batch(*L.call(), L.arr, L.N, self._mode(), int(self.clamp_scales))
        _lib.check(rc, "GaussianMixtureConditional.estimate_bits")
        items = L.items
        cols = zip(items["bits_q"].tolist(), items["bytes_pred"].tolist(), items["n_symbols"].tolist(), items["n_bypass"].tolist(),
                   items["abs_max"].tolist(), bitmaps, chans, maps)
        return [RateEstimate(*c) for c in cols]

    def estimate_bits(self, y: Tensor, scales: Tensor, means: Tensor, weights: Tensor, *, weights_are_logits: bool = False,
                      per_channel: bool = False, per_latent: bool = False) -> RateEstimate:
        """-> the ``RateEstimate`` of ``compress(y, scales, means, weights)``: its size, without coding"""
        return self.estimate_bits_batch([y], [scales], [means], [weights], weights_are_logits=weights_are_logits, per_channel=per_channel,
                                        per_latent=per_latent)[0]

    def reconstruct_batch(self, y_hats, scales, means, weights, *, weights_are_logits: bool = False, p_min: float = 2.0 ** -16,
                          return_kept: bool = False):
        """Centroid reconstruction of decoded latents (include/flashgmm_amd.h section 3i): per latent the conditional mean of its bin
        ``[q - 1/2, q + 1/2)`` under its mixture, which minimises the expected squared LATENT error - the decoder-side twin of
        ``quantize_rdo_batch``, at no bit and with no change of format.  What it buys in the image domain depends on the trained
        synthesis transform and is not claimed.  A latent whose bin has a likelihood below ``p_min`` (default: the coder's resolution),
        whose offset would leave the bin or whose terms are not finite keeps ``round(y_hat)``.  One kernel; the scale bound is the
        module's ``scale_bound``, as in ``forward``.  Inputs as ``estimate_bits_batch`` takes them - sequences of ``[1, M, h, w]`` /
        ``[1, K*M, h, w]`` tensors, or stacked; no autograd, the inputs are detached.  -> per item the float32 reconstruction
        ``[1, M, h, w]``, or ``(reconstruction, n_kept)`` with ``return_kept`` - ``n_kept`` the latents that left the integer grid."""
        self._check_k()
        p_min = float(p_min)
        if not 0.0 < p_min < float("inf"):
            raise ValueError(f"p_min = {p_min!r}: must be positive and finite")
        detach = lambda t: t.detach() if isinstance(t, Tensor) else [x.detach() for x in t]  # noqa: E731
        L = self._latent_items(_lib.fgmm_centroid_item, *(detach(t) for t in (y_hats, scales, means, weights)), weights_are_logits)
        if L.N == 0:
            return []
        recs = L.output("rec", torch.float32, per_latent=True)
        rc = _lib.lib().fgmm_gmc_centroid_batch(*L.call(), L.arr, L.N, self.scale_bound, p_min)
        _lib.check(rc, "GaussianMixtureConditional.reconstruct")
        return list(zip(recs, L.items["n_kept"].tolist())) if return_kept else list(recs)

    def reconstruct(self, y_hat: Tensor, scales: Tensor, means: Tensor, weights: Tensor, *, weights_are_logits: bool = False,
                    p_min: float = 2.0 ** -16, return_kept: bool = False):
        """-> the centroid reconstruction of one decoded latent (``reconstruct_batch``), ``(rec, n_kept)`` with ``return_kept``"""
        return self.reconstruct_batch([y_hat], [scales], [means], [weights], weights_are_logits=weights_are_logits, p_min=p_min,
                                      return_kept=return_kept)[0]

    def quantize_rdo_batch(self, ys, scales, means, weights, lam: float, *, weights_are_logits: bool = False,
                           per_channel: bool = False, channel_weights=None, position_weights=None, channel_skip: bool = False) -> List[RdoQuantized]:
        """Rate-distortion optimised quantisation: per latent of a channel ``compress_batch`` would code, ``round(y)`` or one of its
        two neighbours, whichever minimises ``(y - v)**2 + lam * bits(v)`` - ``bits`` the coder's own exact cost of ``v`` under that
        latent's mixture (the rule, exactly: include/flashgmm_amd.h section 3c).  One kernel; nothing is coded.  Inputs as
        ``compress_batch`` takes them - sequences of ``[1, M, h, w]`` / ``[1, K*M, h, w]`` tensors, or stacked; ``lam`` finite, >= 0
        (0 returns ``round(y)``).  -> one ``RdoQuantized`` per item; ``compress(result.y, ...)`` then codes it through the unchanged
        encode path.

        ``channel_weights`` / ``position_weights`` (section 3e) weight the squared error of the latent at channel ``c``, position ``p``
        by ``channel_weights[c] * position_weights[p]``: float32 tensors on the latents' device, every factor finite and in
        ``[0, 256]``.  ``channel_weights``: ``[M]`` shared by the batch, or a sequence of one (or None) per item.
        ``position_weights``: ``[h, w]`` or ``[1, 1, h, w]`` per item, or ``[N, 1, h, w]`` for stacked input.  None, or arrays of
        ones: exactly the unweighted result.

        ``channel_skip`` (section 3f): after the per-latent decisions a coded channel is dropped whole where that lowers the
        objective; -> ``RdoSkipQuantized``.  False changes nothing."""
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        lam = float(lam)
        if not (0.0 <= lam < float("inf")):
            raise ValueError(f"lam = {lam!r}: must be finite and >= 0")
        wl = _rdo_weight_lists(ys, channel_weights, position_weights)
        flags = _lib.FGMM_PARAMS_LOGITS if weights_are_logits else 0
        if wl is None and not channel_skip and isinstance(ys, Tensor):  # the plain stacked call: no item array on this side
            y, scales, means, weights, N, M, h, w, s_item, sc = self._stacked_view(ys, scales, means, weights)
            if N == 0:
                return []
            dev = scales.device
            out = torch.empty((N, 1, M, h, w), dtype=torch.float32, device=dev)
            zb = torch.empty((N, M), dtype=torch.int64)
            cb = torch.empty((N, M), dtype=torch.int64) if per_channel else None
            ch, before, after, am = _lib.boundary().rdoq_stacked(*_ctx_stream(dev), y.data_ptr(), scales.data_ptr(),
                                                                 means.data_ptr(), weights.data_ptr(), N, M, h * w, s_item, M * sc, sc,
                                                                 _abi_dtype(scales.dtype), flags, self._mode(),
                                                                 int(self.clamp_scales), lam, out.data_ptr(), zb.data_ptr(), cb.data_ptr() if per_channel else 0)
            return [RdoQuantized(*c) for c in zip(out.unbind(0), ch, before, after, am, zb.unbind(0), cb.unbind(0) if per_channel else [None] * N)]
        L = self._latent_items(_lib.fgmm_rdoq_item, ys, scales, means, weights, weights_are_logits)
        if L.N == 0:
            return []
        outs, bitmaps = L.output("y_rdo", torch.float32, per_latent=True), L.output("zero_bitmap", torch.int64)
        chans = L.output("chan_bits_q_after", torch.int64) if per_channel else [None] * L.N
        warr = _rdo_weights_array(wl)
        sarr, sflags = _rdo_skip_array(L, per_channel) if channel_skip else (None, None)
        _lib.boundary().rdoq_items(*L.call(), C.addressof(L.arr), L.N, self._mode(), int(self.clamp_scales), lam, _addr(warr), _addr(sarr))
        items = L.items
        cols = zip(outs, items["n_changed"].tolist(), items["bits_q_before"].tolist(), items["bits_q_after"].tolist(), items["abs_max"].tolist(),
                   bitmaps, chans)
        if channel_skip:
            return [RdoSkipQuantized(*c, sk) for c, sk in zip(cols, _rdo_skip_cols(sarr, sflags))]
        return [RdoQuantized(*c) for c in cols]

    def quantize_rdo(self, y: Tensor, scales: Tensor, means: Tensor, weights: Tensor, lam: float, *, weights_are_logits: bool = False,
                     per_channel: bool = False, channel_weights=None, position_weights=None, channel_skip: bool = False) -> RdoQuantized:
        """-> the ``RdoQuantized`` of one latent (``quantize_rdo_batch``)"""
        return self.quantize_rdo_batch([y], [scales], [means], [weights], lam, weights_are_logits=weights_are_logits, per_channel=per_channel,
                                       channel_weights=channel_weights, position_weights=_one_item(position_weights), channel_skip=channel_skip)[0]

    def _latent_items(self, struct, ys, scales, means, weights, logits: bool) -> _LatentItems:
        """THE item builder of the calls that price latents (estimate, RDOQ, curve, budget): ``struct[N]`` with the input fields
        set - stacked tensors column by column (``_stacked_view``, ``_boundary.fill_items``: one validation, the pointers batch-dimension
        offsets), sequences through ``_item_ints`` item by item"""
        flags = _lib.FGMM_PARAMS_LOGITS if logits else 0
        if isinstance(ys, Tensor):
            y, s, m, wt, N, M, h, w, s_item, sc = self._stacked_view(ys, scales, means, weights)
            L = _LatentItems(struct, N, [y, s, m, wt], s.device, shape=(1, M, h, w))
            _boundary.fill_items(L.items, s.data_ptr(), m.data_ptr(), wt.data_ptr(), s_item, M * sc, sc, _abi_dtype(s.dtype), flags, M, h * w, y.data_ptr())
            return L
        L = _LatentItems(struct, len(ys), [], ys=ys)
        keep, dev = L.keep, None
        for i, it in enumerate(L.arr):
            yp, sp, mp, wp, M, hw, sk, sc, d, dt = self._item_ints(ys[i], scales[i], means[i], weights[i], keep)
            dev = dev or d
            if d != dev:
                raise RuntimeError("all items of a batch must be on one device")
            it.y = yp
            it.params = _lib.fgmm_params(sp, mp, wp, sk, sc, dt, flags)
            it.M, it.K, it.hw = M, self.K, hw
        L.dev = dev
        return L

    def rd_curve_batch(self, ys, scales, means, weights, lambdas, *, weights_are_logits: bool = False, channel_weights=None,
                       position_weights=None, channel_skip: bool = False) -> List[RdCurve]:
        """What ``quantize_rdo_batch`` would report at every lambda of ``lambdas`` - the cost after, the latents moved, the distortion
        added - WITHOUT quantising: one kernel prices each latent once and decides it at up to 16 lambdas (include/flashgmm_amd.h
        section 3d); more are served in chunks of 16.  Inputs as ``quantize_rdo_batch`` takes them; ``lambdas`` finite, >= 0, in any
        order.  ``channel_weights`` / ``position_weights``: as ``quantize_rdo_batch`` takes them - the curve is then the weighted
        call's, ``ddist_q`` the weighted added distortion.  ``channel_skip``: what ``quantize_rdo_batch(channel_skip=True)`` would
        report, with ``n_skipped`` per lambda (section 3f).  -> one ``RdCurve`` per item."""
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        lambdas = [float(v) for v in lambdas]
        if not lambdas or not all(0.0 <= v < float("inf") for v in lambdas):
            raise ValueError(f"lambdas = {lambdas!r}: at least one, each finite and >= 0")
        wl = _rdo_weight_lists(ys, channel_weights, position_weights)
        L = self._latent_items(_lib.fgmm_rdcurve_item, ys, scales, means, weights, weights_are_logits)
        if L.N == 0:
            return []
        call, items, warr = _lib.boundary().rdcurve_items, L.items, _rdo_weights_array(wl)
        names = ("bits_q_after", "n_changed", "ddist_q")
        cols = [[] for _ in names]
        sarr = (_lib.fgmm_rdcurve_skip * L.N)() if channel_skip else None
        n_skipped = [[] for _ in range(L.N)]
        for at in range(0, len(lambdas), _lib.FGMM_RDCURVE_MAX):
            chunk = lambdas[at:at + _lib.FGMM_RDCURVE_MAX]
            call(*L.call(), C.addressof(L.arr), L.N, self._mode(), int(self.clamp_scales), chunk, _addr(warr), _addr(sarr))
            for i in range(L.N if channel_skip else 0):
                n_skipped[i].extend(sarr[i].n_skipped[:len(chunk)])
            for col, name in zip(cols, names):
                col.append(items[name][:, :len(chunk)].copy())
        cols = [np.concatenate(col, axis=1).tolist() for col in cols]
        return [RdCurve(lambdas, *c) for c in zip(items["bits_q_before"].tolist(), *cols, items["n_symbols"].tolist(),
                                                  n_skipped if channel_skip else [None] * L.N,
                                                  [a.n_eligible for a in sarr] if channel_skip else [None] * L.N)]

    def rd_curve(self, y: Tensor, scales: Tensor, means: Tensor, weights: Tensor, lambdas, *, weights_are_logits: bool = False,
                 channel_weights=None, position_weights=None, channel_skip: bool = False) -> RdCurve:
        """-> the ``RdCurve`` of one latent (``rd_curve_batch``)"""
        return self.rd_curve_batch([y], [scales], [means], [weights], lambdas, weights_are_logits=weights_are_logits,
                                   channel_weights=channel_weights, position_weights=_one_item(position_weights), channel_skip=channel_skip)[0]

    def quantize_to_budget_batch(self, ys, scales, means, weights, budget_bytes, *, groups=None, lambda_max: float = 16.0, refine: int = 2,
                                 weights_are_logits: bool = False, per_channel: bool = False, channel_weights=None,
                                 position_weights=None, channel_skip: bool = False) -> List[BudgetQuantized]:
        """Rate-distortion optimised quantisation TO A BYTE BUDGET: lambda is searched on the rate-distortion curve by the fixed rule of
        include/flashgmm_amd.h section 3d - a 16-point grid 0, lambda_max * 2^-14 .. lambda_max, then ``refine`` (0..8) rounds of 16
        points between the last infeasible and the first feasible one, each round one pass of the curve kernel - then ``quantize_rdo_batch``'s
        result at the lambda found.  ``groups``: one group id per item, 0 .. n_groups - 1 - the items of a group share one lambda and
        one budget on the sum of their bytes (None: every item its own group).  ``budget_bytes``: an int for all groups, or one per
        group.  -> one ``BudgetQuantized`` per item (an ``RdoQuantized`` that carries ``lam``, ``bytes_pred``, ``budget_met``, ``passes``
        of its group).  The budget is on PREDICTED bytes: a real stream may be 4 bytes longer where ``estimate_bits`` may be off;
        a channel the quantisation empties is no longer coded, so on that account the real size can only be smaller.
        ``channel_weights`` / ``position_weights``: as ``quantize_rdo_batch`` takes them - the search is the same, the decisions it
        sums and the final quantisation are the weighted ones.  ``channel_skip`` (section 3f): the search runs over the curve after
        the channel decisions and ends in ``quantize_rdo_batch(channel_skip=True)``; an emptied channel then counts nothing."""
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        lambda_max, refine = float(lambda_max), int(refine)
        if not (0.0 < lambda_max < float("inf")):
            raise ValueError(f"lambda_max = {lambda_max!r}: must be finite and > 0")
        if not 0 <= refine <= 8:
            raise ValueError(f"refine = {refine!r}: must lie in 0 .. 8")
        wl = _rdo_weight_lists(ys, channel_weights, position_weights)
        L = self._latent_items(_lib.fgmm_rdoq_item, ys, scales, means, weights, weights_are_logits)
        N, items, warr = L.N, L.items, _rdo_weights_array(wl)
        if groups is not None:
            groups = [int(g) for g in groups]
            if len(groups) != N:
                raise ValueError(f"groups: one id per item ({N}), got {len(groups)}")
            n_groups = max(groups, default=-1) + 1
            if min(groups, default=0) < 0 or set(groups) != set(range(n_groups)):
                raise ValueError("groups: ids must be 0 .. n_groups - 1 with no group empty")
        else:
            n_groups = N
        if isinstance(budget_bytes, (list, tuple)):
            budgets = [int(b) for b in budget_bytes]
            if len(budgets) != n_groups:
                raise ValueError(f"budget_bytes: one per group ({n_groups}), got {len(budgets)}")
        else:
            budgets = [int(budget_bytes)] * n_groups
        if any(b < 0 for b in budgets):
            raise ValueError("budget_bytes must be >= 0")
        if N == 0:
            return []
        outs, bitmaps = L.output("y_rdo", torch.float32, per_latent=True), L.output("zero_bitmap", torch.int64)
        chans = L.output("chan_bits_q_after", torch.int64) if per_channel else [None] * N
        sarr, sflags = _rdo_skip_array(L, per_channel) if channel_skip else (None, None)
        res = _lib.boundary().rdoq_budget_items(*L.call(), C.addressof(L.arr), N, self._mode(), int(self.clamp_scales), groups, budgets,
                                                lambda_max, refine, _addr(warr), _addr(sarr))
        got = []
        cols = zip(outs, items["n_changed"].tolist(), items["bits_q_before"].tolist(), items["bits_q_after"].tolist(), items["abs_max"].tolist(),
                   bitmaps, chans)
        skips = _rdo_skip_cols(sarr, sflags) if channel_skip else [None] * N
        for i, c in enumerate(cols):
            lam, nbytes, passes, status = res[groups[i] if groups is not None else i]
            got.append(BudgetQuantized(*c, float(lam), int(nbytes), status != _lib.FGMM_BUDGET_UNMET, int(passes), skips[i]))
        return got

    def quantize_to_budget(self, y: Tensor, scales: Tensor, means: Tensor, weights: Tensor, budget_bytes: int, *, lambda_max: float = 16.0,
                           refine: int = 2, weights_are_logits: bool = False, per_channel: bool = False, channel_weights=None,
                           position_weights=None, channel_skip: bool = False) -> BudgetQuantized:
        """-> the ``BudgetQuantized`` of one latent (``quantize_to_budget_batch``)"""
        return self.quantize_to_budget_batch([y], [scales], [means], [weights], budget_bytes, lambda_max=lambda_max, refine=refine,
                                             weights_are_logits=weights_are_logits, per_channel=per_channel, channel_weights=channel_weights,
                                             position_weights=_one_item(position_weights), channel_skip=channel_skip)[0]

    def compress(self, y: Tensor, scales: Tensor, means: Tensor, weights: Tensor, *, weights_are_logits: bool = False):
        """-> ((bytes, abs_max, zero_bitmap), y_quantized)     (entropy_models.py:833-867)"""
        ((data, abs_max, zb), yq), = self.compress_batch([y], [scales], [means], [weights], weights_are_logits=weights_are_logits)
        return (data, abs_max, zb.to(y.device)), yq

    def decompress_batch(self, strings: Sequence[bytes], abs_maxes: Sequence[int], zero_bitmaps, scales, means,
                         weights, *, weights_are_logits: bool = False, stacked_output: bool = False):
        """N independent ``decompress`` calls in one native call; parameters as sequences of ``[1, K*M, h, w]``
        tensors or stacked ``[N, K*M, h, w]`` (see ``compress_batch``; ``zero_bitmaps`` may then be one ``[N, M]`` tensor).
        Returns N ``[1, M, h, w]`` tensors - with ``stacked_output`` (stacked parameters only) the one ``[N, 1, M, h, w]``
        tensor they are views of."""
        if self.K != _lib.FGMM_K:
            raise RuntimeError(f"K = {self.K}: the coder is bound for K = 4 only (as the reference's)")
        flags = _lib.FGMM_PARAMS_LOGITS if weights_are_logits else 0
        if isinstance(scales, Tensor):
            return self._decompress_stacked(strings, abs_maxes, zero_bitmaps, scales, means, weights, flags, stacked_output)
        if stacked_output:
            raise RuntimeError("stacked_output needs stacked parameters ([N, K*M, h, w] tensors)")
        n_items = len(strings)
        if n_items == 0:
            return []
        keep, tuples, outs, dev = [], [], [], None  # the items as tuples of integers (fgmm_pybind.cpp: decompress_items)
        for i in range(n_items):
            _, sp, mp, wp, M, hw, sk, sc, d, dt = self._item_ints(None, scales[i], means[i], weights[i], keep)
            dev = dev or d
            if d != dev:
                raise RuntimeError("all items of a batch must be on one device")
            zb = zero_bitmaps[i]
            if zb.device.type != "cpu" or zb.dtype != torch.int64 or not zb.is_contiguous():
                zb = zb.to("cpu", torch.int64).contiguous()
            if zb.numel() != M:
                raise RuntimeError(f"zero_bitmap has {zb.numel()} entries, expected {M}")
            shp = scales[i].shape
            y_hat = torch.empty((1, M, shp[2], shp[3]), dtype=torch.float32, device=d)
            keep.append(zb)
            outs.append(y_hat)
            tuples.append((sp, mp, wp, M, hw, sk, sc, y_hat.data_ptr(), zb.data_ptr(), dt))
        data = strings if isinstance(strings, list) and all(isinstance(s_, bytes) for s_ in strings) else [s_ if isinstance(s_, bytes) else bytes(s_) for s_ in strings]
        _lib.boundary().decompress_items(*_ctx_stream(dev), data, [int(a) for a in abs_maxes], tuples, flags, self._mode(),
                                         int(self.clamp_scales), CheckpointedBytes)
        return outs

    def decompress(self, strings: bytes, abs_max: int, zero_bitmap: Tensor, scales: Tensor, means: Tensor,
                   weights: Tensor, *, weights_are_logits: bool = False) -> Tensor:
        """-> y_hat [1, M, h, w] float32     (entropy_models.py:872-910)"""
        return self.decompress_batch([strings], [abs_max], [zero_bitmap], [scales], [means], [weights],
                                     weights_are_logits=weights_are_logits)[0]


class EntropyBottleneckCoder(nn.Module):
    """The coding half of the reference's ``EntropyBottleneck`` (compressai/entropy_models/entropy_models.py:605-618 over
    ``EntropyModel.compress / decompress``, :237-327) for the `z` hyper-latent, given the tables its ``update()`` built:

        coder = EntropyBottleneckCoder.from_entropy_bottleneck(eb)      # any object with the reference's buffers
        strings = coder.compress(z)                                     # list of bytes, one per batch element
        z_hat = coder.decompress(strings, z.shape[-2:])                 # [N, C, h, w] on the tables' device

    Same bytes as the reference for the same tables and the same ``z`` (golden G5 / G8); what differs is the plumbing:
    the reference turns the symbol tensor, the index tensor AND the whole CDF matrix into Python lists on every call
    (:257-266); here the tables are converted once, the symbols cross as one int32 copy, and the indexes (channel of
    every element, ``_build_indexes`` :555-566) are built once per shape.  Integer work on the host, as the reference's;
    the learned density model behind the tables (``_likelihood``, ``update()``) stays the caller's (stock CompressAI)."""

    def __init__(self, quantized_cdf: Tensor, cdf_length: Tensor, offset: Tensor, medians: Tensor):
        super().__init__()
        from .ans import _Tables

        if quantized_cdf.dim() != 2 or cdf_length.dim() != 1 or offset.dim() != 1:
            raise ValueError("expected _quantized_cdf [C, L], _cdf_length [C], _offset [C] (run update() first)")
        self.channels = int(quantized_cdf.size(0))
        if cdf_length.numel() != self.channels or offset.numel() != self.channels or medians.numel() != self.channels:
            raise ValueError("tables and medians must describe the same number of channels")
        self._tables = _Tables(quantized_cdf.detach().cpu().numpy(), cdf_length.detach().cpu().numpy(), offset.detach().cpu().numpy())
        self.register_buffer("medians", medians.detach().reshape(-1).to(torch.float32).clone())
        self._index_cache = {}

    @classmethod
    def from_entropy_bottleneck(cls, eb) -> "EntropyBottleneckCoder":
        """``eb``: the reference's (or stock CompressAI's) ``EntropyBottleneck`` after ``update()``"""
        return cls(eb._quantized_cdf, eb._cdf_length, eb._offset, eb.quantiles[:, 0, 1])

    def _indexes(self, spatial: int) -> np.ndarray:
        idx = self._index_cache.get(spatial)
        if idx is None:
            idx = np.repeat(np.arange(self.channels, dtype=np.int32), spatial)
            self._index_cache[spatial] = idx
        return idx

    def compress(self, x: Tensor, return_dequantized: bool = False):
        """-> list of bytes, one per batch element; with ``return_dequantized`` also what ``decompress`` of those strings
        yields — ``quantize(x) + medians`` computed where ``x`` lives (:158-176, :197-204: the coder is lossless on the
        int32 symbols, so decoding them back is one elementwise op, not a host encode -> host decode -> upload)."""
        if x.dim() < 2 or x.size(1) != self.channels:
            raise ValueError(f"expected [N, {self.channels}, ...], got {tuple(x.shape)}")
        med = self.medians.to(x.device).reshape(1, -1, *([1] * (x.dim() - 2)))
        # quantize(inputs, "symbols", means): round(x - means).int()  (:158-176) — on the tensor's device, ONE copy out
        sym_dev = torch.round(x - med).to(torch.int32)
        sym = sym_dev.reshape(x.size(0), -1).cpu().numpy()
        if return_dequantized:
            return self._encode_rows(sym), sym_dev.to(torch.float32) + med  # dequantize: outputs.type_as(means) + means
        return self._encode_rows(sym)

    def _encode_rows(self, sym: np.ndarray) -> List[bytes]:
        idx = self._indexes(sym.shape[1] // self.channels)
        L = _lib.lib()
        out = []
        for i in range(sym.shape[0]):
            row = np.ascontiguousarray(sym[i])
            o, n = C.c_void_p(), C.c_size_t()
            _lib.check(L.fgmm_encode_with_indexes(row.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), row.size,
                                                  *self._tables.args(), C.byref(o), C.byref(n)), "EntropyBottleneck.compress")
            out.append(_lib.take_bytes(o, n.value))
        return out

    def decompress(self, strings: Sequence[bytes], size) -> Tensor:
        if not isinstance(strings, (tuple, list)):
            raise ValueError("Invalid `strings` parameter type.")
        size = tuple(int(v) for v in size)
        spatial = int(np.prod(size)) if size else 1
        idx = self._indexes(spatial)
        L = _lib.lib()
        sym = np.empty((len(strings), idx.size), np.int32)
        for i, sdata in enumerate(strings):
            sdata = bytes(sdata)
            _lib.check(L.fgmm_decode_with_indexes(sdata, len(sdata), idx.ctypes.data_as(C.c_void_p), idx.size, *self._tables.args(),
                                                  sym[i].ctypes.data_as(C.c_void_p)), "EntropyBottleneck.decompress")
        dev = self.medians.device
        med = self.medians.reshape(1, -1, *([1] * len(size)))
        # dequantize(outputs, means): outputs.type_as(means) + means  (:197-204)
        return torch.from_numpy(sym).to(dev).reshape(len(strings), self.channels, *size).to(torch.float32) + med


# ---- the entropy bottleneck's density model (include/flashgmm_amd.h section 3j) ---------------------------------------------------------
class _EbLikelihoodFn(torch.autograd.Function):
    """``EntropyBottleneck.forward`` / ``rate_bits`` on the GPU (section 3j): one kernel forward; a backward kernel that recomputes both
    chains from the inputs and a small one that sums its rows - nothing but the inputs is saved.  ``x`` ``[B, C, hw]`` float32 contiguous,
    ``theta`` ``[C, 58]`` float32 (the raw parameters in the header's order), ``med`` ``[C]``.  ``mode`` 1: the kernel dequantizes
    (``rintf(x - med) + med``); 0: ``x`` is the already-noised value.  -> ``(main, v, n_nonfinite)`` as ``_LikelihoodFn``'s."""

    @staticmethod
    def forward(ctx, x, theta, med, mode: int, want_map: bool, lb: float):
        B, Cn, hw = x.shape
        theta, med = theta.contiguous(), med.contiguous()
        like = torch.empty_like(x) if want_map else None
        v = torch.empty_like(x) if mode else None
        bits_q, nonfinite = np.zeros(B, np.int64), np.zeros(B, np.int64)
        call = _lib.fgmm_eb_call(x.data_ptr(), theta.data_ptr(), med.data_ptr(), B, Cn, hw, like.data_ptr() if want_map else None,
                                 v.data_ptr() if mode else None, bits_q.ctypes.data, nonfinite.ctypes.data, 0, 0)
        _lib.check(_lib.lib().fgmm_eb_likelihood(*_ctx_stream(x.device), C.byref(call), int(mode), lb), "EntropyBottleneck.forward")
        ctx.save_for_backward(x, theta, med)
        ctx.mode, ctx.want_map, ctx.lb = int(mode), want_map, lb
        nonfinite = torch.from_numpy(nonfinite)
        ctx.mark_non_differentiable(nonfinite)
        if v is not None:
            ctx.mark_non_differentiable(v)
        main = like if want_map else torch.from_numpy(bits_q.astype(np.float64) * 2.0 ** -_lib.FGMM_LIKE_Q).to(x.device)
        return main, v, nonfinite

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_main, g_v, g_nonfinite):
        x, theta, med = ctx.saved_tensors
        need_x, need_t, need_m = ctx.needs_input_grad[:3]
        need_x, need_m = need_x and not ctx.mode, need_m and bool(ctx.mode)  # round() has gradient zero; the noised path does not see med
        if g_main is None or not (need_x or need_t or need_m):
            return (None,) * 6
        B, Cn, hw = x.shape
        dx = torch.empty_like(x) if need_x else None
        dtheta = torch.empty_like(theta) if need_t else None
        dmed = torch.empty_like(med) if need_m else None
        g = g_bits = None
        if ctx.want_map:
            g = g_main.to(torch.float32).contiguous()  # (held until the call returns: the call waits for its kernels)
        else:
            g_bits = np.ascontiguousarray(g_main.detach().to("cpu", torch.float64).numpy())
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        call = _lib.fgmm_eb_grad_call(x.data_ptr(), theta.data_ptr(), med.data_ptr(), B, Cn, hw, ptr(g),
                                      None if g_bits is None else g_bits.ctypes.data, ptr(dx), ptr(dtheta), ptr(dmed), 0, 0)
        _lib.check(_lib.lib().fgmm_eb_likelihood_backward(*_ctx_stream(x.device), C.byref(call), ctx.mode, ctx.lb),
                   "EntropyBottleneck.forward (backward)")
        return dx, dtheta, dmed, None, None, None


class _EbBound(nn.Module):
    """holds the ``bound`` buffer of the reference's ``likelihood_lower_bound`` (bound_ops.py:71), so that state dicts carry the same keys"""

    def __init__(self, bound: float):
        super().__init__()
        self.register_buffer("bound", torch.Tensor([float(bound)]))


class EntropyBottleneck(nn.Module):
    """The reference's ``EntropyBottleneck`` (compressai/entropy_models/entropy_models.py:330-510) with its density model on the GPU:
    same parameters (``_matrix{i}``, ``_bias{i}``, ``_factor{i}``, ``quantiles``), buffers and initialisation, so that a reference
    checkpoint loads with ``strict=True``; ``forward`` / ``rate_bits`` run the fused kernels of include/flashgmm_amd.h section 3j, which
    form the likelihood in the mirrored form (the reference's written form is rounding noise in the upper tail in float32).  The kernels
    are bound to ``filters=(3, 3, 3, 3)``, the reference's default and what both GMM models construct.  ``update()`` builds the tables
    (header section 3k): the support from the quantiles as the reference does, the masses by the kernels in ``forward``'s own arithmetic,
    so that a model trained here is coded here; ``update_quantiles=True`` bisects the quantiles first, every channel on its own.  Tables
    define the bitstream: a decoder uses the ones its encoder used, which is why they travel in the state dict.  ``coder()`` codes on them."""

    FILTERS = (3, 3, 3, 3)
    _TABLES = ("_offset", "_quantized_cdf", "_cdf_length")

    def __init__(self, channels: int, tail_mass: float = 1e-9, init_scale: float = 10, filters: Tuple[int, ...] = (3, 3, 3, 3),
                 likelihood_bound: float = 1e-9):
        super().__init__()
        self.channels, self.filters = int(channels), tuple(int(f) for f in filters)
        self.init_scale, self.tail_mass, self.likelihood_bound = float(init_scale), float(tail_mass), float(likelihood_bound)
        if self.filters != self.FILTERS:
            raise ValueError(f"filters = {self.filters}: the kernels are bound to the reference's default {self.FILTERS}")
        if self.channels < 1:
            raise ValueError("channels must be at least 1")
        if not 0.0 <= self.likelihood_bound < float("inf"):
            raise ValueError("likelihood_bound must be finite and >= 0 (0: no bound)")
        self.use_likelihood_bound = self.likelihood_bound > 0
        if self.use_likelihood_bound:
            self.likelihood_lower_bound = _EbBound(self.likelihood_bound)
        for name in self._TABLES:  # filled by update(), or by a checkpoint of an updated model
            self.register_buffer(name, torch.IntTensor())
        self.update_report = None  # update(): {"pmf_length": [C], "tail_mass": [C]}
        width = (1,) + self.filters + (1,)
        scale = self.init_scale ** (1 / (len(self.filters) + 1))
        for i in range(len(self.filters) + 1):  # :360-385
            self.register_parameter(f"_matrix{i:d}", nn.Parameter(torch.full((self.channels, width[i + 1], width[i]),
                                                                             float(np.log(np.expm1(1 / scale / width[i + 1]))))))
            self.register_parameter(f"_bias{i:d}", nn.Parameter(torch.empty(self.channels, width[i + 1], 1).uniform_(-0.5, 0.5)))
            if i < len(self.filters):
                self.register_parameter(f"_factor{i:d}", nn.Parameter(torch.zeros(self.channels, width[i + 1], 1)))
        self.quantiles = nn.Parameter(torch.tensor([-self.init_scale, 0.0, self.init_scale]).repeat(self.channels, 1, 1))
        target = float(np.log(2 / self.tail_mass - 1))
        self.register_buffer("target", torch.tensor([-target, 0.0, target]))

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for name in self._TABLES:  # the tables arrive with their own sizes
            t = state_dict.get(prefix + name)
            if t is not None and tuple(t.shape) != tuple(getattr(self, name).shape):
                setattr(self, name, torch.empty(tuple(t.shape), dtype=getattr(self, name).dtype, device=getattr(self, name).device))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        if self.use_likelihood_bound:
            self.likelihood_bound = float(self.likelihood_lower_bound.bound.item())
        self.__dict__.pop("_coder_cache", None)

    # ------------------------------------------------------------------------------------------------
    def _get_medians(self) -> Tensor:
        return self.quantiles[:, :, 1:2]

    def _theta(self) -> Tensor:
        """the raw parameters as ONE float32 block ``[C, 58]`` in the header's order (its backward is the one split of the gradient)"""
        parts = []
        for i in range(len(self.filters) + 1):
            parts += [getattr(self, f"_matrix{i:d}"), getattr(self, f"_bias{i:d}")]
            if i < len(self.filters):
                parts.append(getattr(self, f"_factor{i:d}"))
        return torch.cat([p.reshape(self.channels, -1) for p in parts], 1)

    def _logits_cumulative(self, inputs: Tensor, stop_gradient: bool = False) -> Tensor:
        """plain torch on ``[C, 1, n]`` (:434-453): what ``loss`` runs on the three quantiles; the kernels restate it per element"""
        logits = inputs
        for i in range(len(self.filters) + 1):
            names = [f"_matrix{i:d}", f"_bias{i:d}"] + ([f"_factor{i:d}"] if i < len(self.filters) else [])
            m, b, *f = [getattr(self, n).detach() if stop_gradient else getattr(self, n) for n in names]
            logits = torch.matmul(F.softplus(m), logits) + b
            if f:
                logits = logits + torch.tanh(f[0]) * torch.tanh(logits)
        return logits

    def loss(self) -> Tensor:
        """the quantile loss (:429-432)"""
        return torch.abs(self._logits_cumulative(self.quantiles, stop_gradient=True) - self.target).sum()

    def _prepare(self, x: Tensor, training: Optional[bool]):
        if x.dim() < 2 or x.size(1) != self.channels:
            raise RuntimeError(f"expected [B, {self.channels}, ...], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            raise RuntimeError(f"the hyper-latent must be float32, got {x.dtype}")
        if not x.is_cuda:
            raise RuntimeError("EntropyBottleneck.forward runs on the GPU: the hyper-latent must be a CUDA/HIP tensor (there is no CPU path)")
        if x.numel() == 0:
            raise RuntimeError("the likelihood needs at least one element")
        if training is None:
            training = self.training
        values = x.reshape(x.size(0), x.size(1), -1)
        if training:
            values = values + torch.empty_like(values).uniform_(-0.5, 0.5)  # quantize(values, "noise") (:163-167)
        return values.contiguous(), bool(training), self._theta().to(torch.float32), self._get_medians().reshape(-1).to(torch.float32)

    def likelihood(self, values: Tensor, *, dequantize: bool = False) -> Tuple[Tensor, Tensor]:
        """The building block of ``forward``: -> ``(v, likelihood)`` of ``values`` ``[B, C, ...]`` as they are, or (``dequantize``) of
        ``v = round(values - medians) + medians``.  Differentiable in the parameters and, without rounding, in ``values``."""
        vals, _, theta, med = self._prepare(values, False)
        like, v, _ = _EbLikelihoodFn.apply(vals, theta, med, int(dequantize), True, self.likelihood_bound)
        return (v.reshape(values.shape) if dequantize else values), like.reshape(values.shape)

    def forward(self, x: Tensor, training: Optional[bool] = None) -> Tuple[Tensor, Tensor]:
        """As the reference's (:465-510): -> ``(outputs, likelihood)``, both shaped like ``x`` ``[B, C, ...]`` float32.  ``training``
        (default ``self.training``): ``outputs`` is ``x`` plus uniform noise in [-0.5, 0.5) drawn by torch; otherwise
        ``round(x - medians) + medians``, formed by the kernel (it then carries no gradient)."""
        vals, training, theta, med = self._prepare(x, training)
        like, v, _ = _EbLikelihoodFn.apply(vals, theta, med, int(not training), True, self.likelihood_bound)
        return (vals if training else v).reshape(x.shape), like.reshape(x.shape)

    def rate_bits(self, x: Tensor, training: Optional[bool] = None, return_nonfinite: bool = False):
        """The fused rate of ``forward``, shaped like ``GaussianMixtureConditional.rate_bits``: -> ``(outputs, bits)``, ``bits`` a float64
        ``[B]`` on ``x``'s device - per item ``sum(-log2(likelihood))``, summed on the GPU as integers in units of 2^-32 bit,
        differentiable like the sum it stands for; no map is written.  ``return_nonfinite=True`` adds the count of the elements whose
        likelihood is NaN, infinite or <= 0 (left out of the sum) as an int64 ``[B]`` CPU tensor."""
        vals, training, theta, med = self._prepare(x, training)
        bits, v, nonfinite = _EbLikelihoodFn.apply(vals, theta, med, int(not training), False, self.likelihood_bound)
        outputs = (vals if training else v).reshape(x.shape)
        return (outputs, bits, nonfinite) if return_nonfinite else (outputs, bits)

    # ------------------------------------------------------------------------------------------------
    def _update_device(self) -> torch.device:
        dev = self.quantiles.device
        if dev.type != "cuda":
            raise RuntimeError("EntropyBottleneck.update runs on the GPU: the module must be on a CUDA/HIP device (there is no CPU path)")
        return dev

    def _search_quantiles(self, search_radius: float = 1e5) -> Tensor:
        """-> ``[C, 1, 3]`` float32: per channel and target the bisected solution of ``chain(q) = target`` on ``[-search_radius,
        search_radius]`` (``fgmm_eb_quantiles``, header section 3k; NaN where the chain of a search gave NaN)"""
        dev = self._update_device()
        theta = self._theta().detach().to(torch.float32).contiguous()
        q = torch.empty((self.channels, 3), dtype=torch.float32, device=dev)
        targets = (C.c_float * 3)(*self.target.detach().to("cpu", torch.float32).tolist())
        _lib.check(_lib.lib().fgmm_eb_quantiles(*_ctx_stream(dev), theta.data_ptr(), self.channels, targets, float(search_radius), q.data_ptr()),
                   "EntropyBottleneck._update_quantiles")
        return q.reshape(self.channels, 1, 3)

    @torch.no_grad()
    def _update_quantiles(self, search_radius: float = 1e5) -> None:
        """the reference's fast quantile update (:572-603) as one kernel: every channel's three searches run to the end on their own,
        where the reference stops all channels once all pass ``isclose(rtol=1e-4, atol=1e-3)``"""
        self.quantiles.copy_(self._search_quantiles(search_radius))

    @torch.no_grad()
    def update(self, force: bool = False, update_quantiles: bool = False) -> bool:
        """As the reference's (:391-427): builds ``_offset``, ``_quantized_cdf`` ``[C, max_length + 2]`` and ``_cdf_length`` (int32, on the
        module's device) from the quantiles, after bisecting those anew with ``update_quantiles``; -> False, nothing done, when the tables
        are there and ``force`` is not set.  The support is the reference's float32 / int32 arithmetic in torch; the masses are the
        kernels' (``fgmm_eb_tables``, header section 3k: the mirrored form, bit for bit ``forward``'s unbounded likelihood of the
        same points; each channel's tail at its own last sample), the integer quantiser the host's.  The module changes only once the call has
        succeeded: a channel whose quantiles are not finite, whose support exceeds 2^16 counts or whose masses are invalid raises
        ``ValueError`` naming it.  ``update_report``: per channel ``pmf_length`` and ``tail_mass`` (the mass the tail entry holds);
        a tail above ``10 * tail_mass`` - quantiles that do not bracket the density, as untrained ones do not - is warned about."""
        if self._offset.numel() > 0 and not force:
            return False
        dev = self._update_device()
        q = (self._search_quantiles() if update_quantiles else self.quantiles.detach()).to(torch.float32)
        bad = (~torch.isfinite(q)).reshape(self.channels, -1).any(1).nonzero()
        if bad.numel():
            raise ValueError(f"EntropyBottleneck.update: channel {int(bad[0])}: its quantiles {q[int(bad[0]), 0].tolist()} are not finite")
        medians = q[:, 0, 1]
        span = torch.clamp(torch.ceil(medians - q[:, 0, 0]).double(), min=0) + torch.clamp(torch.ceil(q[:, 0, 2] - medians).double(), min=0) + 2
        bad = (span > 65536).nonzero()
        if bad.numel():
            raise ValueError(f"EntropyBottleneck.update: channel {int(bad[0])}: {int(span[int(bad[0])])} symbols (its support and the tail) "
                             "exceed 2^16 counts")
        minima = torch.clamp(torch.ceil(medians - q[:, 0, 0]).int(), min=0)
        maxima = torch.clamp(torch.ceil(q[:, 0, 2] - medians).int(), min=0)
        pmf_start = (medians - minima).contiguous()
        pmf_length = (maxima + minima + 1).contiguous()
        stride = int(pmf_length.max().item()) + 1
        theta = self._theta().detach().to(torch.float32).contiguous()
        pmf = torch.empty((self.channels, stride), dtype=torch.float32, device=dev)
        cdf = np.zeros((self.channels, stride + 1), np.int32)
        failed = C.c_int32(-1)
        rc = _lib.lib().fgmm_eb_tables(*_ctx_stream(dev), theta.data_ptr(), pmf_start.data_ptr(), pmf_length.data_ptr(), self.channels, stride,
                                       pmf.data_ptr(), cdf.ctypes.data, C.byref(failed))
        if rc == 1 and failed.value >= 0:  # FGMM_ERR_INVALID with a channel named: a property of the model, not of the call
            raise ValueError("EntropyBottleneck.update: " + _lib.lib().fgmm_last_error().decode(errors="replace"))
        _lib.check(rc, "EntropyBottleneck.update")
        tail = pmf.gather(1, pmf_length.long().reshape(-1, 1)).reshape(-1).cpu()
        if update_quantiles:
            self.quantiles.copy_(q)
        self._offset = -minima
        self._quantized_cdf = torch.from_numpy(cdf).to(dev)
        self._cdf_length = pmf_length + 2
        self.__dict__.pop("_coder_cache", None)
        self.update_report = {"pmf_length": pmf_length.cpu().tolist(), "tail_mass": tail.tolist()}
        over = (tail > 10 * self.tail_mass).nonzero().reshape(-1).tolist()
        if over:
            warnings.warn(f"EntropyBottleneck.update: the tail entry of {len(over)} of {self.channels} channels holds more than 10 * tail_mass "
                          f"(channel {over[0]}: {float(tail[over[0]]):.3g}): the quantiles do not bracket the density; "
                          "update(force=True, update_quantiles=True) bisects them first", stacklevel=3)
        return True

    def coder(self) -> "EntropyBottleneckCoder":
        """the coding half on this module's table buffers (built once per state of tables and medians)"""
        if any(getattr(self, n).numel() == 0 for n in self._TABLES):
            raise RuntimeError("the table buffers are empty: load the checkpoint of an updated model, or run update()")
        key = tuple(k for n in self._TABLES for k in (getattr(self, n)._version, getattr(self, n).data_ptr())) + (self.quantiles._version, self.quantiles.data_ptr())
        cached = self.__dict__.get("_coder_cache")
        if cached is None or cached[0] != key:
            cached = (key, EntropyBottleneckCoder.from_entropy_bottleneck(self))
            self.__dict__["_coder_cache"] = cached  # (not a registered submodule: its buffer stays out of the state dict)
        return cached[1]

    def compress(self, x: Tensor):
        return self.coder().compress(x)

    def decompress(self, strings, size) -> Tensor:
        return self.coder().decompress(strings, size)


def update_entropy_models(module: nn.Module, force: bool = False, update_quantiles: bool = False) -> bool:
    """``CompressionModel.update`` (compressai/models/base.py:117-141) for any module tree: ``update()`` of every ``EntropyBottleneck``
    in it (``module`` itself included) -> whether at least one was updated.  (The GMM path has no scale table to update.)"""
    updated = False
    for m in module.modules():
        if isinstance(m, EntropyBottleneck):
            updated |= m.update(force=force, update_quantiles=update_quantiles)
    return updated


def aux_loss(module: nn.Module) -> Tensor:
    """``CompressionModel.aux_loss`` (base.py:143-172): the sum of the quantile losses of every ``EntropyBottleneck`` of the tree (the
    integer 0 for a tree without one, as the reference's ``sum``)"""
    return sum(m.loss() for m in module.modules() if isinstance(m, EntropyBottleneck))
