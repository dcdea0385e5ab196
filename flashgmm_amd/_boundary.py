"""The stand-in for ``flashgmm_amd._native`` where the compiled module cannot be used (``_lib.boundary()``): the same nine callables,
parameter for parameter and result for result, over the ctypes binding of ``_lib``.  csrc/fgmm_pybind.cpp documents the interface; what
differs is the binding's own: no sink (``fgmm_gmc_compress_batch``, then ``fgmm_ctx_take_buffers`` into the bytes objects), the GIL as
ctypes handles it, and ``_lib.FgmmError`` (a RuntimeError) for a status.  Contexts, streams, device and host memory arrive as integer
addresses; nothing here touches a tensor."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_py = C.pythonapi
_py.PyBytes_FromStringAndSize.restype = C.py_object
_py.PyBytes_FromStringAndSize.argtypes = [C.c_void_p, C.c_ssize_t]
_py.PyBytes_AsString.restype = C.c_void_p
_py.PyBytes_AsString.argtypes = [C.py_object]


_DTYPES = {_lib.fgmm_item: _lib.ITEM_DTYPE, _lib.fgmm_rdoq_item: _lib.RDOQ_ITEM_DTYPE}


def records(struct, n: int):
    """-> (``struct[n]`` as ctypes passes it, zeroed; the same memory as a numpy record array, filled and read column by column)"""
    arr = (struct * n)()
    return arr, np.frombuffer(arr, _DTYPES[struct])


def _at(addr: int, struct):
    return C.cast(addr, C.POINTER(struct)) if addr else None


def fill_items(items, scales, means, weights, item_stride, stride_k, stride_c, dtype, flags, M, hw, y=0):
    """fill_items of fgmm_pybind.cpp: the input fields of N stacked items (records of ``fgmm_item`` or of an item type that begins
    alike): item i of a plane = base + i * item_stride elements (an absent plane, base 0, stays null), ``y`` dense float32
    -> arange(N) as uint64, for the columns the caller adds"""
    rng = np.arange(len(items), dtype=np.uint64)
    step = rng * np.uint64(item_stride * (4 if dtype == _lib.FGMM_F32 else 2))
    for name, base in (("scales", scales), ("means", means), ("weights", weights)):
        if base:
            items[name] = np.uint64(base) + step
    items["stride_k"], items["stride_c"], items["dtype"], items["flags"] = stride_k, stride_c, dtype, flags
    items["M"], items["K"], items["hw"] = M, _lib.FGMM_K, hw
    if y:
        items["y"] = np.uint64(y) + rng * np.uint64(M * hw * 4)
    return rng


def sequence_items(tuples, at: int, flags: int):
    """item_common of fgmm_pybind.cpp: ``fgmm_item[]`` from the tuples of the sequence form, whose fields from ``at`` on are
    (scales, means, weights, M, hw, stride_k, stride_c, yq / y_hat, zero_bitmap, dtype) -> ``records``"""
    arr, items = records(_lib.fgmm_item, len(tuples))
    names = ("y",)[:at] + ("scales", "means", "weights", "M", "hw", "stride_k", "stride_c", "yq_out", "zero_bitmap", "dtype")
    for t in tuples:
        if len(t) != len(names):
            raise RuntimeError(f"an item is ({', '.join(names)})")
    for name, col in zip(names, zip(*tuples)):
        items[name] = col
    items["K"], items["flags"] = _lib.FGMM_K, flags
    return arr, items


def take_bytes_many(ctx: int, ptrs, lens, cls=None) -> list:
    """library-allocated buffers -> ``bytes`` objects (or instances of the bytes subclass ``cls``), the buffers released.
    The copies are done by the context's host workers, straight into the objects' own storage: ``bytes`` objects allocated
    uninitialised (``PyBytes_FromStringAndSize(NULL, n)``: the C API's way to fill a bytes object before anyone else sees it),
    subclass instances as ``bytes.__new__(cls, n)`` (zero pages until written) - one copy, not one per layer of glue."""
    n = len(ptrs)
    if n == 0:
        return []
    if cls is None:
        if sum(lens) < (1 << 18):
            return [_lib.take_bytes(p, l) for p, l in zip(ptrs, lens)]
        objs = [_py.PyBytes_FromStringAndSize(None, int(l)) for l in lens]
    else:
        objs = [bytes.__new__(cls, int(l)) for l in lens]
    dst = (C.c_void_p * n)(*[_py.PyBytes_AsString(o) if l else None for o, l in zip(objs, lens)])
    _lib.check(_lib.lib().fgmm_ctx_take_buffers(ctx, dst, (C.c_void_p * n)(*ptrs), (C.c_size_t * n)(*lens), n), "fgmm_ctx_take_buffers")
    return objs


def _adopt_ckpts(ctx: int, items, strings, ckpt_stride: int) -> None:
    """adopt_ckpts of fgmm_pybind.cpp: ONE bytes object takes every item's notes back to back (16 bytes each; the library's arrays
    are released) and every bitstream object gets its ``_ck`` = (blob, first record, records, address of the first, stride)"""
    counts = [n if p and n > 0 else 0 for p, n in zip(items["ckpt"].tolist(), items["n_ckpt"].tolist())]
    blob = _py.PyBytes_FromStringAndSize(None, 16 * sum(counts))
    base, first, dst, src = _py.PyBytes_AsString(blob), 0, [], []
    for b, p, n in zip(strings, items["ckpt"].tolist(), counts):
        b._ck = (blob, first, n, base + 16 * first if n else 0, ckpt_stride)
        if n:
            dst.append(base + 16 * first), src.append(p)
        first += n
    if dst:
        n, lens = len(dst), [16 * c for c in counts if c]
        rc = _lib.lib().fgmm_ctx_take_buffers(ctx, (C.c_void_p * n)(*dst), (C.c_void_p * n)(*src), (C.c_size_t * n)(*lens), n)
        _lib.check(rc, "fgmm_ctx_take_buffers")


def _stacked_outputs(items, rng, M, hw, yq, zero_bitmap, zb_row_stride, ckpt_stride=None):
    items["yq_out"] = np.uint64(yq) + rng * np.uint64(M * hw * 4)
    items["zero_bitmap"] = np.uint64(zero_bitmap) + rng * np.uint64(zb_row_stride * 8)
    if ckpt_stride is not None:
        items["ckpt_stride"] = ckpt_stride


def _finish_compress(ctx, items, ckpt_stride, bytes_cls):
    strings = take_bytes_many(ctx, items["bytes"].tolist(), items["bytes_len"].tolist(), bytes_cls)
    if ckpt_stride:
        _adopt_ckpts(ctx, items, strings, ckpt_stride)
    return strings, items["abs_max"].tolist()


def _borrow(items, strings, abs_maxes, ckpt_cls):
    """the bitstreams of a decompress call, read in place, and the notes of those that carry them (instances of ``ckpt_cls``: ``_ck``)
    -> what must stay alive across the call"""
    for i, b in enumerate(strings):
        if not isinstance(b, bytes):
            raise RuntimeError(f"decompress: bitstream {i} is not a bytes object")
    keep = (list(strings), (C.c_char_p * len(strings))(*strings))  # borrowed pointers into the bytes objects
    items["bytes"], items["bytes_len"] = np.frombuffer(keep[1], dtype=np.uint64), [len(b) for b in strings]
    items["abs_max"] = np.asarray(abs_maxes, dtype=np.int64)
    if ckpt_cls is not None and any(isinstance(b, ckpt_cls) for b in strings):
        cks = [b._ck[2:5] if isinstance(b, ckpt_cls) else (0, 0, 0) for b in strings]  # (count, address, stride)
        items["n_ckpt"], items["ckpt"], items["ckpt_stride"] = zip(*cks)
    return keep


def compress_stacked(ctx, stream, y, scales, means, weights, N, M, hw, item_stride, stride_k, stride_c, dtype, flags, mode, clamp_scales,
                     ckpt_stride, yq, zero_bitmap, bytes_cls=None):
    arr, items = records(_lib.fgmm_item, N)
    rng = fill_items(items, scales, means, weights, item_stride, stride_k, stride_c, dtype, flags, M, hw, y)
    _stacked_outputs(items, rng, M, hw, yq, zero_bitmap, M, ckpt_stride)
    _lib.check(_lib.lib().fgmm_gmc_compress_batch(ctx, stream, arr, N, mode, clamp_scales), "GaussianMixtureConditional.compress")
    return _finish_compress(ctx, items, ckpt_stride, bytes_cls)


def compress_head_stacked(ctx, stream, y, x, head, N, M, c_in, hw, mode, clamp_scales, ckpt_stride, yq, zero_bitmap, bytes_cls=None):
    arr, items = records(_lib.fgmm_item, N)
    rng = fill_items(items, 0, 0, 0, 0, 0, 0, _lib.FGMM_F32, _lib.FGMM_PARAMS_LOGITS, M, hw, y)
    _stacked_outputs(items, rng, M, hw, yq, zero_bitmap, M, ckpt_stride)
    xs = (C.c_void_p * N)(*[x + i * c_in * hw * 4 for i in range(N)])
    _lib.check(_lib.lib().fgmm_gmc_compress_head_batch(ctx, stream, arr, xs, N, head, mode, clamp_scales), "GaussianMixtureConditional.compress_head_batch")
    return _finish_compress(ctx, items, ckpt_stride, bytes_cls)


def decompress_stacked(ctx, stream, strings, abs_maxes, zero_bitmap, zb_row_stride, scales, means, weights, N, M, hw, item_stride, stride_k,
                       stride_c, dtype, flags, mode, clamp_scales, y_hat, ckpt_cls=None):
    if len(strings) != N or len(abs_maxes) != N:
        raise RuntimeError(f"decompress: {N} items in the parameter tensors, {len(strings)} bitstreams")
    arr, items = records(_lib.fgmm_item, N)
    rng = fill_items(items, scales, means, weights, item_stride, stride_k, stride_c, dtype, flags, M, hw)
    _stacked_outputs(items, rng, M, hw, y_hat, zero_bitmap, zb_row_stride)
    alive = _borrow(items, strings, abs_maxes, ckpt_cls)
    _lib.check(_lib.lib().fgmm_gmc_decompress_batch(ctx, stream, arr, N, mode, clamp_scales), "GaussianMixtureConditional.decompress")
    del alive


def compress_items(ctx, stream, items, flags, mode, clamp_scales, ckpt_stride, bytes_cls=None):
    arr, rec = sequence_items(items, 1, flags)
    rec["ckpt_stride"] = ckpt_stride
    _lib.check(_lib.lib().fgmm_gmc_compress_batch(ctx, stream, arr, len(arr), mode, clamp_scales), "GaussianMixtureConditional.compress")
    return _finish_compress(ctx, rec, ckpt_stride, bytes_cls)


def decompress_items(ctx, stream, strings, abs_maxes, items, flags, mode, clamp_scales, ckpt_cls=None):
    if len(strings) != len(items) or len(abs_maxes) != len(items):
        raise RuntimeError(f"decompress: {len(items)} items, {len(strings)} bitstreams")
    arr, rec = sequence_items(items, 0, flags)
    alive = _borrow(rec, strings, abs_maxes, ckpt_cls)
    _lib.check(_lib.lib().fgmm_gmc_decompress_batch(ctx, stream, arr, len(arr), mode, clamp_scales), "GaussianMixtureConditional.decompress")
    del alive


def rdoq_stacked(ctx, stream, y, scales, means, weights, N, M, hw, item_stride, stride_k, stride_c, dtype, flags, mode, clamp_scales, lam,
                 y_rdo, zero_bitmap, chan_after=0):
    arr, items = records(_lib.fgmm_rdoq_item, N)
    rng = fill_items(items, scales, means, weights, item_stride, stride_k, stride_c, dtype, flags, M, hw, y)
    items["y_rdo"] = np.uint64(y_rdo) + rng * np.uint64(M * hw * 4)
    items["zero_bitmap"] = np.uint64(zero_bitmap) + rng * np.uint64(M * 8)
    if chan_after:
        items["chan_bits_q_after"] = np.uint64(chan_after) + rng * np.uint64(M * 8)
    _lib.check(_lib.lib().fgmm_gmc_rdoq_batch(ctx, stream, arr, N, mode, clamp_scales, lam), "GaussianMixtureConditional.quantize_rdo")
    return tuple(items[name].tolist() for name in ("n_changed", "bits_q_before", "bits_q_after", "abs_max"))


def rdoq_items(ctx, stream, items, count, mode, clamp_scales, lam, weights=0, skip=0):
    rc = _lib.lib().fgmm_gmc_rdoq_batch_s(ctx, stream, _at(items, _lib.fgmm_rdoq_item), count, mode, clamp_scales, lam,
                                          _at(weights, _lib.fgmm_rdo_weights), _at(skip, _lib.fgmm_rdo_skip))
    _lib.check(rc, "GaussianMixtureConditional.quantize_rdo")


def rdcurve_items(ctx, stream, items, count, mode, clamp_scales, lambdas, weights=0, skip=0):
    rc = _lib.lib().fgmm_gmc_rdcurve_batch_s(ctx, stream, _at(items, _lib.fgmm_rdcurve_item), count, mode, clamp_scales,
                                             (C.c_double * len(lambdas))(*lambdas), len(lambdas), _at(weights, _lib.fgmm_rdo_weights),
                                             _at(skip, _lib.fgmm_rdcurve_skip))
    _lib.check(rc, "GaussianMixtureConditional.rd_curve")


def rdoq_budget_items(ctx, stream, items, count, mode, clamp_scales, groups, budgets, lambda_max, refine, weights=0, skip=0):
    res = (_lib.fgmm_budget_result * len(budgets))()
    rc = _lib.lib().fgmm_gmc_rdoq_budget_batch_s(ctx, stream, _at(items, _lib.fgmm_rdoq_item), count, mode, clamp_scales,
                                                 (C.c_int32 * count)(*groups) if groups is not None else None, len(budgets),
                                                 (C.c_uint64 * len(budgets))(*budgets), lambda_max, refine, res, _at(weights, _lib.fgmm_rdo_weights),
                                                 _at(skip, _lib.fgmm_rdo_skip))
    _lib.check(rc, "GaussianMixtureConditional.quantize_to_budget")
    return [(r.lambda_, r.bytes_pred, r.passes, r.status) for r in res]
