"""ctypes binding of libflashgmm_amd.so (include/flashgmm_amd.h).

The library is built in-tree by ``flashgmm_amd/csrc/build.sh`` (``__graft_entry__.build()``).  There is no
Python or CPU fallback for it: if the shared object is missing or no HIP device is usable, every entry point
raises — loudly — instead of silently doing the work some other way.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FGMM_LIB") or os.path.join(HERE, "libflashgmm_amd.so")  # FGMM_LIB: A/B builds (dev)

FGMM_OK = 0
FGMM_HOST, FGMM_DEVICE = 0, 1
FGMM_K = 4
FGMM_F32, FGMM_F16, FGMM_BF16 = 0, 1, 2
FGMM_HEAD_BF16X6 = 1  # fgmm_head_create_ex flags
FGMM_PARAMS_LOGITS = 1  # fgmm_params.flags: the weights planes hold logits, softmax over K runs in the kernels
MODES = {"polya": 0, "as": 1, "logistic": 2}  # numbering of the reference CODE (rans_interface.cpp:224-232)

FGMM_BUDGET_UNMET = 7  # fgmm_budget_result.status: not an error - no lambda up to lambda_max meets the group's byte budget
FGMM_RDCURVE_MAX = 16  # lambdas per fgmm_gmc_rdcurve_batch call
FGMM_RDO_W_MAX = 256.0  # largest factor of a weighted call's chan_w / pos_w (section 3e)
STATUS_NAMES = {1: "FGMM_ERR_INVALID", 2: "FGMM_ERR_NO_DEVICE", 3: "FGMM_ERR_HIP", 4: "FGMM_ERR_NOMEM",
                5: "FGMM_ERR_STREAM", 6: "FGMM_ERR_UNSUPPORTED"}


class FgmmError(RuntimeError):
    """Raised for every non-zero fgmm_status (the reference raises RuntimeError through pybind11 as well)."""


class fgmm_params(C.Structure):
    _fields_ = [("scales", C.c_void_p), ("means", C.c_void_p), ("weights", C.c_void_p),
                ("stride_k", C.c_int64), ("stride_c", C.c_int64), ("dtype", C.c_int32), ("flags", C.c_int32)]


class fgmm_ckpt(C.Structure):
    _fields_ = [("x", C.c_uint64), ("pos", C.c_uint64)]


class fgmm_call_marks(C.Structure):
    _fields_ = [("kind", C.c_int32), ("count", C.c_int32), ("t_begin_ms", C.c_double), ("ms", C.c_double * 6),
                ("worker_busy_ms", C.c_double), ("worker_wait_ms", C.c_double), ("head_ms", C.c_double * 3)]


class fgmm_item(C.Structure):
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("yq_out", C.c_void_p), ("zero_bitmap", C.c_void_p), ("abs_max", C.c_int32),
                ("bytes", C.c_void_p), ("bytes_len", C.c_size_t), ("status", C.c_int32), ("ckpt_stride", C.c_int32),
                ("ckpt", C.c_void_p), ("n_ckpt", C.c_int64)]


class fgmm_rate_item(C.Structure):
    """one item of fgmm_gmc_estimate_batch (include/flashgmm_amd.h section 3b)"""
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("zero_bitmap", C.c_void_p), ("chan_bits_q", C.c_void_p), ("bits_map", C.c_void_p), ("abs_max", C.c_int32),
                ("status", C.c_int32), ("n_symbols", C.c_int64), ("n_bypass", C.c_int64), ("bits_q", C.c_uint64), ("bytes_pred", C.c_uint64)]


class fgmm_rdoq_item(C.Structure):
    """one item of fgmm_gmc_rdoq_batch (include/flashgmm_amd.h section 3c)"""
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("y_rdo", C.c_void_p), ("zero_bitmap", C.c_void_p), ("chan_bits_q_after", C.c_void_p), ("abs_max", C.c_int32),
                ("status", C.c_int32), ("n_changed", C.c_int64), ("bits_q_before", C.c_uint64), ("bits_q_after", C.c_uint64)]


class fgmm_rdcurve_item(C.Structure):
    """one item of fgmm_gmc_rdcurve_batch (include/flashgmm_amd.h section 3d)"""
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("bits_q_before", C.c_uint64), ("bits_q_after", C.c_uint64 * FGMM_RDCURVE_MAX), ("n_changed", C.c_uint64 * FGMM_RDCURVE_MAX),
                ("ddist_q", C.c_uint64 * FGMM_RDCURVE_MAX), ("n_symbols", C.c_int64), ("status", C.c_int32), ("pad_", C.c_int32)]


class fgmm_budget_result(C.Structure):
    """one group's result of fgmm_gmc_rdoq_budget_batch (section 3d)"""
    _fields_ = [("lambda_", C.c_double), ("bytes_pred", C.c_uint64), ("passes", C.c_int32), ("status", C.c_int32)]


class fgmm_rdo_weights(C.Structure):
    """one item's factors of the weighted calls (section 3e): device float32 ``chan_w[M]`` / ``pos_w[hw]``, either may be null"""
    _fields_ = [("chan_w", C.c_void_p), ("pos_w", C.c_void_p)]


class fgmm_rdo_skip(C.Structure):
    """one item's outputs of channel skipping (section 3f): host int64 ``skipped[M]`` (may be null), the counts, the added distortion"""
    _fields_ = [("skipped", C.c_void_p), ("n_skipped", C.c_int64), ("n_eligible", C.c_int64), ("ddist_q", C.c_uint64)]


class fgmm_rdcurve_skip(C.Structure):
    """one item's outputs of channel skipping on the curve (section 3f)"""
    _fields_ = [("n_skipped", C.c_uint64 * FGMM_RDCURVE_MAX), ("n_eligible", C.c_int64)]


class fgmm_like_item(C.Structure):
    """one item of fgmm_gmc_likelihood_batch (include/flashgmm_amd.h section 3g)"""
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("like_out", C.c_void_p), ("v_out", C.c_void_p), ("bits_q", C.c_int64), ("n_nonfinite", C.c_int64),
                ("status", C.c_int32), ("pad_", C.c_int32)]


class fgmm_like_grad_item(C.Structure):
    """one item of fgmm_gmc_likelihood_backward_batch (section 3g)"""
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("g_like", C.c_void_p), ("g_bits", C.c_double), ("dy", C.c_void_p), ("dscales", C.c_void_p), ("dmeans", C.c_void_p),
                ("dweights", C.c_void_p), ("status", C.c_int32), ("pad_", C.c_int32)]


class fgmm_centroid_item(C.Structure):
    """one item of fgmm_gmc_centroid_batch (include/flashgmm_amd.h section 3i)"""
    _fields_ = [("y", C.c_void_p), ("params", fgmm_params), ("M", C.c_int32), ("K", C.c_int32), ("hw", C.c_int64),
                ("rec", C.c_void_p), ("n_kept", C.c_int64), ("status", C.c_int32), ("pad_", C.c_int32)]


class fgmm_eb_call(C.Structure):
    """the call structure of fgmm_eb_likelihood (include/flashgmm_amd.h section 3j); ``bits_q`` / ``n_nonfinite``: HOST int64 ``[B]``"""
    _fields_ = [("x", C.c_void_p), ("theta", C.c_void_p), ("med", C.c_void_p), ("B", C.c_int32), ("C", C.c_int32), ("hw", C.c_int64),
                ("like_out", C.c_void_p), ("v_out", C.c_void_p), ("bits_q", C.c_void_p), ("n_nonfinite", C.c_void_p),
                ("status", C.c_int32), ("pad_", C.c_int32)]


class fgmm_eb_grad_call(C.Structure):
    """the call structure of fgmm_eb_likelihood_backward (section 3j); ``g_bits``: HOST float64 ``[B]``, read when ``g_like`` is null"""
    _fields_ = [("x", C.c_void_p), ("theta", C.c_void_p), ("med", C.c_void_p), ("B", C.c_int32), ("C", C.c_int32), ("hw", C.c_int64),
                ("g_like", C.c_void_p), ("g_bits", C.c_void_p), ("dx", C.c_void_p), ("dtheta", C.c_void_p), ("dmed", C.c_void_p),
                ("status", C.c_int32), ("pad_", C.c_int32)]


def _item_dtype(struct=fgmm_item):
    """numpy view of ``fgmm_item[]`` (offsets taken from the ctypes declaration): lets a batch be filled column by
    column instead of field by field."""
    import numpy as np
    names, formats, offsets = [], [], []
    kinds = {C.c_void_p: "<u8", C.c_int64: "<i8", C.c_int32: "<i4", C.c_size_t: "<u8", C.c_uint64: "<u8", C.c_double: "<f8"}
    for name, typ in struct._fields_:
        base = getattr(struct, name).offset
        if typ is fgmm_params:
            for pn, pt in fgmm_params._fields_:
                names.append(pn); formats.append(kinds[pt]); offsets.append(base + getattr(fgmm_params, pn).offset)
        elif issubclass(typ, C.Array):
            names.append(name); formats.append((kinds[typ._type_], (typ._length_,))); offsets.append(base)
        else:
            names.append(name); formats.append(kinds[typ]); offsets.append(base)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": C.sizeof(struct)})


ITEM_DTYPE = _item_dtype()
RATE_ITEM_DTYPE = _item_dtype(fgmm_rate_item)
RDOQ_ITEM_DTYPE = _item_dtype(fgmm_rdoq_item)
RDCURVE_ITEM_DTYPE = _item_dtype(fgmm_rdcurve_item)
LIKE_ITEM_DTYPE = _item_dtype(fgmm_like_item)
LIKE_GRAD_ITEM_DTYPE = _item_dtype(fgmm_like_grad_item)
CENTROID_ITEM_DTYPE = _item_dtype(fgmm_centroid_item)
FGMM_EB_PARAMS = 58  # float32 values per channel of section 3j's theta
FGMM_EB_SLICE = 1024  # section 3j: elements of a channel one workgroup walks
FGMM_EB_SEARCH_CAP = 256  # section 3k: bisection steps of one quantile search at the most
FGMM_LIKE_Q = 32  # unit of the likelihood call's bits_q: 2^-32 bit
FGMM_RATE_Q = 24  # unit of the size estimate's costs: 2^-24 bit

SINK_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_size_t)  # fgmm_sink.alloc(user, item, nbytes) -> address


class fgmm_sink(C.Structure):
    """where a batched compress call puts its bitstreams (include/flashgmm_amd.h); alloc is called on the calling thread, inside
    the native call (ctypes takes the GIL back for a Python callback by itself)"""
    _fields_ = [("alloc", SINK_ALLOC), ("user", C.c_void_p)]


# every symbol include/flashgmm_amd.h declares: (restype, argtypes)
_p, _i, _i32, _i64, _sz = C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_size_t
_pp, _psz = C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)
SIGNATURES = {
    "fgmm_abi_version": (_i, []),
    "fgmm_last_error": (C.c_char_p, []),
    "fgmm_host_cpu_budget": (_i, [C.POINTER(C.c_double), C.POINTER(_i), C.POINTER(C.c_double)]),
    "fgmm_host_thread_budget": (_i, [_i]),
    "fgmm_ctx_create": (_i, [_i, _i, _pp]),
    "fgmm_ctx_destroy": (None, [_p]),
    "fgmm_ctx_device": (_i, [_p]),
    "fgmm_ctx_threads": (_i, [_p]),
    "fgmm_ctx_set_threads": (_i, [_p, _i]),
    "fgmm_ctx_worker_cpus": (_i, [_p, C.c_char_p, _sz]),
    "fgmm_free": (None, [_p]),
    "fgmm_ctx_take_buffers": (_i, [_p, _p, _p, _p, _i]),
    "fgmm_ctx_set_profiling": (_i, [_p, _i]),
    "fgmm_ctx_kernel_ms": (_i, [_p, _i, C.POINTER(C.c_float)]),
    "fgmm_ctx_stat": (_i, [_p, _i, C.POINTER(C.c_uint64)]),
    "fgmm_ctx_call_log": (_i, [_p, C.POINTER(fgmm_call_marks), _i, C.POINTER(_i)]),
    "fgmm_encode_with_indexes_gmm": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _i, _i, _i32, _pp, _psz]),
    "fgmm_decode_with_indexes_gmm": (_i, [_p, _p, _sz, _p, _p, _p, _i64, _i64, _i64, _i, _i, _i, _i32, _p]),
    "fgmm_gmc_compress": (_i, [_p, _p, _p, C.POINTER(fgmm_params), _i, _i, _i64, _i, _i, _p, C.POINTER(_i32), _p, _pp, _psz]),
    "fgmm_gmc_decompress": (_i, [_p, _p, _p, _sz, _i32, _p, C.POINTER(fgmm_params), _i, _i, _i64, _i, _i, _p]),
    "fgmm_gmc_compress_batch": (_i, [_p, _p, C.POINTER(fgmm_item), _i, _i, _i]),
    "fgmm_gmc_decompress_batch": (_i, [_p, _p, C.POINTER(fgmm_item), _i, _i, _i]),
    "fgmm_gmc_compress_batch_to": (_i, [_p, _p, C.POINTER(fgmm_item), _i, _i, _i, C.POINTER(fgmm_sink)]),
    "fgmm_head_create": (_i, [_p, _p, _p, _p, _i, _i, _i, _pp]),
    "fgmm_head_create_ex": (_i, [_p, _p, _p, _p, _i, _i, _i, _i, _pp]),
    "fgmm_head_destroy": (None, [_p]),
    "fgmm_head_params_batch": (_i, [_p, _p, _p, _p, _p, _p, _i]),
    "fgmm_gmc_compress_head_batch": (_i, [_p, _p, C.POINTER(fgmm_item), _p, _i, _p, _i, _i]),
    "fgmm_gmc_compress_head_batch_to": (_i, [_p, _p, C.POINTER(fgmm_item), _p, _i, _p, _i, _i, C.POINTER(fgmm_sink)]),
    "fgmm_gmm_cdf_hip": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _p, _p]),
    "fgmm_softmax4_hip": (_i, [_p, _p, _p, _p, _i64]),
    "fgmm_build_symtab_hip": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _p]),
    "fgmm_build_cdftab_hip": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _i32, _i, _p, _p, C.c_uint64, _p]),
    "fgmm_selftest_saturation": (_i, [_p, _i, C.POINTER(C.c_uint64)]),
    "fgmm_selftest_fastmath": (_i, [_p, _i, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    "fgmm_rans_encode_symtab": (_i, [_p, _p, _i64, _pp, _psz]),
    "fgmm_ckpt_count": (_i64, [_i64, _i64]),
    "fgmm_rans_encode_symtab_ckpt": (_i, [_p, _p, _i64, _i64, _pp, _psz, _p]),
    "fgmm_rans_decode_tab_ckpt": (_i, [_p, _sz, _p, _i, _p, _i32, _p, C.c_uint64, _i64, _i32, _i, _p, _i64, _i64, _p, C.POINTER(_i32)]),
    "fgmm_rans_encode_symtab2": (_i, [_p, _p, _i64, _p, _p, _i64, _pp, _psz, _pp, _psz]),
    "fgmm_rans_encode_symtab_n": (_i, [_i, _p, _p, _p, _p, _p]),
    "fgmm_rans_encode_symtab_segs": (_i, [_p, _i, _i64, _p, _i64, _i64, _pp, _psz, _p]),
    "fgmm_rans_decode_cdftab": (_i, [_p, _sz, _p, _p, C.c_uint64, _i64, _i32, _i, _p]),
    "fgmm_rans_decode_tab": (_i, [_p, _sz, _p, _i, _p, _i32, _p, C.c_uint64, _i64, _i32, _i, _p]),
    "fgmm_symtab_bits": (_i, [_p, _p, _i64, _p, C.POINTER(C.c_uint64), C.POINTER(_i64)]),
    "fgmm_rate_stream_bytes": (C.c_uint64, [C.c_uint64]),
    "fgmm_symtab_bits_hip": (_i, [_p, _p, _p, _p, _i64, _p, _p, _p]),
    "fgmm_gmc_estimate_batch": (_i, [_p, _p, C.POINTER(fgmm_rate_item), _i, _i, _i]),
    "fgmm_gmc_rdoq_batch": (_i, [_p, _p, C.POINTER(fgmm_rdoq_item), _i, _i, _i, C.c_double]),
    "fgmm_gmc_rdcurve_batch": (_i, [_p, _p, C.POINTER(fgmm_rdcurve_item), _i, _i, _i, C.POINTER(C.c_double), _i]),
    "fgmm_gmc_rdoq_budget_batch": (_i, [_p, _p, C.POINTER(fgmm_rdoq_item), _i, _i, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_uint64), C.c_double, _i,
                                        C.POINTER(fgmm_budget_result)]),
    "fgmm_gmc_rdoq_batch_w": (_i, [_p, _p, C.POINTER(fgmm_rdoq_item), _i, _i, _i, C.c_double, C.POINTER(fgmm_rdo_weights)]),
    "fgmm_gmc_rdcurve_batch_w": (_i, [_p, _p, C.POINTER(fgmm_rdcurve_item), _i, _i, _i, C.POINTER(C.c_double), _i, C.POINTER(fgmm_rdo_weights)]),
    "fgmm_gmc_rdoq_budget_batch_w": (_i, [_p, _p, C.POINTER(fgmm_rdoq_item), _i, _i, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_uint64), C.c_double, _i,
                                          C.POINTER(fgmm_budget_result), C.POINTER(fgmm_rdo_weights)]),
    "fgmm_gmc_rdoq_batch_s": (_i, [_p, _p, C.POINTER(fgmm_rdoq_item), _i, _i, _i, C.c_double, C.POINTER(fgmm_rdo_weights), C.POINTER(fgmm_rdo_skip)]),
    "fgmm_gmc_rdcurve_batch_s": (_i, [_p, _p, C.POINTER(fgmm_rdcurve_item), _i, _i, _i, C.POINTER(C.c_double), _i, C.POINTER(fgmm_rdo_weights),
                                      C.POINTER(fgmm_rdcurve_skip)]),
    "fgmm_gmc_rdoq_budget_batch_s": (_i, [_p, _p, C.POINTER(fgmm_rdoq_item), _i, _i, _i, C.POINTER(C.c_int32), _i, C.POINTER(C.c_uint64), C.c_double, _i,
                                          C.POINTER(fgmm_budget_result), C.POINTER(fgmm_rdo_weights), C.POINTER(fgmm_rdo_skip)]),
    "fgmm_gmc_likelihood_batch": (_i, [_p, _p, C.POINTER(fgmm_like_item), _i, _i, C.c_float, C.c_float]),
    "fgmm_gmc_likelihood_backward_batch": (_i, [_p, _p, C.POINTER(fgmm_like_grad_item), _i, _i, C.c_float, C.c_float]),
    "fgmm_gmc_likelihood_logits_batch": (_i, [_p, _p, C.POINTER(fgmm_like_item), _i, _i, C.c_float, C.c_float]),
    "fgmm_gmc_likelihood_logits_backward_batch": (_i, [_p, _p, C.POINTER(fgmm_like_grad_item), _i, _i, C.c_float, C.c_float]),
    "fgmm_gmc_centroid_batch": (_i, [_p, _p, C.POINTER(fgmm_centroid_item), _i, C.c_float, C.c_float]),
    "fgmm_eb_likelihood": (_i, [_p, _p, C.POINTER(fgmm_eb_call), _i, C.c_float]),
    "fgmm_eb_likelihood_backward": (_i, [_p, _p, C.POINTER(fgmm_eb_grad_call), _i, C.c_float]),
    # section 3k: (ctx, stream, theta, C, targets[3], search_radius, q_out); (ctx, stream, theta, start, length, C, stride, pmf_out, cdf_out,
    # failed_channel_out)
    "fgmm_eb_quantiles": (_i, [_p, _p, _p, _i, C.POINTER(C.c_float), C.c_float, _p]),
    "fgmm_eb_tables": (_i, [_p, _p, _p, _p, _p, _i, _i, _p, _p, C.POINTER(_i32)]),
    "fgmm_build_tab_hip": (_i, [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _i32, _i, _p, _p, _p, C.c_uint64, _p, C.POINTER(_i32)]),
    "fgmm_ctx_set_option": (_i, [_p, C.c_char_p, _i64]),
    "fgmm_ctx_get_option": (_i, [_p, C.c_char_p, C.POINTER(_i64)]),
    "fgmm_ctx_trim": (_i, [_p]),
    # table path (z hyper-latent coder), host only
    "fgmm_encode_with_indexes": (_i, [_p, _p, _i64, _p, _i64, _i32, _p, _p, _pp, _psz]),
    "fgmm_decode_with_indexes": (_i, [_p, _sz, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "fgmm_symbuf_create": (_i, [_pp]),
    "fgmm_symbuf_destroy": (None, [_p]),
    "fgmm_symbuf_size": (_i64, [_p]),
    "fgmm_symbuf_append_table": (_i, [_p, _p, _p, _i64, _p, _i64, _i32, _p, _p]),
    "fgmm_symbuf_append_symtab": (_i, [_p, _p, _p, _i64]),
    "fgmm_symbuf_flush": (_i, [_p, _pp, _psz]),
    "fgmm_symbuf_append_gmm": (_i, [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i, _i, _i]),
    "fgmm_decstream_create": (_i, [_p, _sz, _pp]),
    "fgmm_decstream_destroy": (None, [_p]),
    "fgmm_decstream_decode": (_i, [_p, _p, _i64, _p, _i64, _i32, _p, _p, _p]),
    "fgmm_pmf_to_quantized_cdf": (_i, [_p, _i, _i, _p]),
    "fgmm_ckbd_unembed": (_i, [_p, _p, _p, _p, _i64, _i64, _i64, _i, _i]),
    "fgmm_ckbd_embed": (_i, [_p, _p, _p, _p, _i64, _i64, _i64, _i, _i]),
    "fgmm_ckbd_ctx_create": (_i, [_p, _p, _p, _p, _i, _i, _pp]),
    "fgmm_ckbd_ctx_destroy": (None, [_p]),
    "fgmm_ckbd_ctx_apply": (_i, [_p, _p, _p, _p, _p, _i, _i64, _i64, _i]),
    # section 5c: (M, C_out); (ctx, stream, weight, bias, M, C_out, transposed, packed); (ctx, stream, packed, M, C_out, anchors, out, n, h, w,
    # anchor_odd); (M, C_out, n, h, w); (ctx, stream, anchors, g, M, C_out, n, h, w, anchor_odd, dweight, dbias, workspace, workspace_bytes)
    "fgmm_ckbd_ctx_packed_floats": (_sz, [_i, _i]),
    "fgmm_ckbd_ctx_pack": (_i, [_p, _p, _p, _p, _i, _i, _i, _p]),
    "fgmm_ckbd_ctx_apply_packed": (_i, [_p, _p, _p, _i, _i, _p, _p, _i, _i64, _i64, _i]),
    "fgmm_ckbd_ctx_wgrad_workspace": (_sz, [_i, _i, _i, _i64, _i64]),
    "fgmm_ckbd_ctx_wgrad": (_i, [_p, _p, _p, _p, _i, _i, _i, _i64, _i64, _i, _p, _p, _p, _sz]),
}
FGMM_CKBD_WGRAD_SLICE_MIN, FGMM_CKBD_WGRAD_SLICES_MAX = 256, 16  # section 5c: the weight gradient's slice rule

_lib = None
_lock = threading.Lock()
_ctxs = {}
_native = None  # flashgmm_amd._native (csrc/fgmm_pybind.cpp), False when it cannot be used


def native():
    """The compiled boundary (``flashgmm_amd._native``, pybind11 over the same C ABI: items built in C++, the GIL released across
    the call) or None - then ``boundary()`` gives the stand-in over this module's ctypes functions.  Not used with FGMM_LIB (an A/B build of the
    library: the module is linked against the in-tree one) or FGMM_NATIVE=0."""
    global _native
    if _native is None:
        _native = False
        if not os.environ.get("FGMM_LIB") and os.environ.get("FGMM_NATIVE", "1") != "0":
            try:
                lib()  # (the library first, by its path: the module's own dependency then resolves to the same mapping)
                from . import _native as mod

                if mod.abi_version == lib().fgmm_abi_version():
                    _native = mod
            except ImportError:
                pass
    return _native or None


def boundary():
    """What ``GaussianMixtureConditional`` makes its batched calls through: ``native()`` or, where that is None, its stand-in
    ``flashgmm_amd._boundary`` - the same callables over this module's ctypes functions.  Looked up at every call."""
    nat = native()
    if nat is not None:
        return nat
    from . import _boundary

    return _boundary


def ctx_addr(device: int = -1) -> int:
    return ctx(device).value


def lib() -> C.CDLL:
    """Load the shared object (no GPU needed for this step) and bind every declared symbol."""
    global _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise FgmmError(
                    f"{LIB_PATH} is missing: build it with flashgmm_amd/csrc/build.sh (or __graft_entry__.build()). "
                    "flashgmm_amd has no CPU / pure-Python fallback for the GMM entropy-coding path."
                )
            L = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(L, name)  # AttributeError here = header and library out of sync
                fn.restype = res
                fn.argtypes = args
            _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != FGMM_OK:
        msg = lib().fgmm_last_error().decode(errors="replace")
        raise FgmmError(f"{what or 'libflashgmm_amd'}: {STATUS_NAMES.get(rc, rc)}: {msg}")


def ctx(device: int = -1, n_threads: int = 0) -> C.c_void_p:
    """Process-wide context of a GPU (created on first use; needs a real HIP device)."""
    L = lib()
    key = int(device)
    with _lock:
        h = _ctxs.get(key)
    if h is None:
        out = C.c_void_p()
        if n_threads <= 0:  # this process's share of the host's CPU budget (affinity mask, cgroup quota, ranks on the node)
            n_threads = L.fgmm_host_thread_budget(ranks_on_node())
        check(L.fgmm_ctx_create(key, int(n_threads), C.byref(out)), "fgmm_ctx_create")
        with _lock:
            if key in _ctxs:  # lost a race: keep the first
                L.fgmm_ctx_destroy(out)
            else:
                _ctxs[key] = out
            h = _ctxs[key]
    return h


def take_bytes(ptr: C.c_void_p, length: int) -> bytes:
    data = C.string_at(ptr, length)
    lib().fgmm_free(ptr)
    return data


def mode_id(mode) -> int:
    if isinstance(mode, str):
        return MODES[mode.lower()]
    m = int(mode)
    if m not in (0, 1, 2):
        raise ValueError(f"mode {mode!r}")
    return m


def default_mode() -> int:
    """APPROX_MODE env var, parsed as the reference does (rans_interface.cpp:99-115): 0/1/2, anything else -> 0."""
    try:
        m = int(os.environ.get("APPROX_MODE", "0"))
    except ValueError:
        return 0
    return m if 0 <= m <= 2 else 0


def set_option(device: int, name: str, value: int) -> None:
    """a tuning knob of the device's context (include/flashgmm_amd.h: fgmm_ctx_set_option)"""
    check(lib().fgmm_ctx_set_option(ctx(device), name.encode(), int(value)), f"fgmm_ctx_set_option({name})")


def get_option(device: int, name: str) -> int:
    out = C.c_int64()
    check(lib().fgmm_ctx_get_option(ctx(device), name.encode(), C.byref(out)), f"fgmm_ctx_get_option({name})")
    return int(out.value)


def trim(device: int) -> None:
    check(lib().fgmm_ctx_trim(ctx(device)), "fgmm_ctx_trim")


def ranks_on_node() -> int:
    """processes (one per GPU) that share this host's CPU budget: LOCAL_WORLD_SIZE as torch.distributed.run exports it (bench.py's
    own launcher exports it too), FGMM_RANKS_ON_NODE to say it by hand; 1 otherwise"""
    for name in ("FGMM_RANKS_ON_NODE", "LOCAL_WORLD_SIZE"):
        try:
            v = int(os.environ.get(name, ""))
            if v >= 1:
                return v
        except ValueError:
            pass
    return 1


def host_cpu_budget() -> dict:
    """-> {"cpus", "affinity", "quota"} (fgmm_host_cpu_budget; quota None when the cgroup sets none)"""
    cpus, aff, quota = C.c_double(), C.c_int(), C.c_double()
    check(lib().fgmm_host_cpu_budget(C.byref(cpus), C.byref(aff), C.byref(quota)), "fgmm_host_cpu_budget")
    return {"cpus": cpus.value, "affinity": aff.value, "quota": quota.value if quota.value > 0 else None}


def set_threads(device: int, n_threads: int) -> None:
    """Resize the pool of host rANS workers of the device's context in place (0: the default for this process's share of the
    host).  Options, profiling state and buffers of the context are kept; the handle from ``ctx()`` stays valid."""
    if n_threads <= 0:
        n_threads = lib().fgmm_host_thread_budget(ranks_on_node())
    check(lib().fgmm_ctx_set_threads(ctx(device), int(n_threads)), "fgmm_ctx_set_threads")


def set_profiling(device: int, enable: bool) -> None:
    check(lib().fgmm_ctx_set_profiling(ctx(device), int(enable)), "fgmm_ctx_set_profiling")


def kernel_ms(device: int, which: int) -> float:
    """Duration (ms) of the most recent launch of kernel `which` (0 symtab, 1 decode-side table kernels of the last call,
    first to last, 2 quant_stats), from HIP events recorded on the stream the kernel ran on."""
    out = C.c_float()
    check(lib().fgmm_ctx_kernel_ms(ctx(device), which, C.byref(out)), "fgmm_ctx_kernel_ms")
    return float(out.value)


def ctx_stat(device: int, which: int) -> int:
    """Counters of the most recent batched call (0 encode tables D2H bytes, 1 decode tables D2H bytes, 2 decode latents,
    3 edges the decode-side kernels evaluated)."""
    out = C.c_uint64()
    check(lib().fgmm_ctx_stat(ctx(device), which, C.byref(out)), "fgmm_ctx_stat")
    return int(out.value)


CALL_KINDS = {0: "encode", 1: "decode", 2: "decode_gpu"}


def worker_cpus(device: int) -> str:
    """cpulist of the CPUs the context's host workers may run on ("" = the creating thread's mask): fgmm_ctx_worker_cpus"""
    buf = C.create_string_buffer(4096)
    check(lib().fgmm_ctx_worker_cpus(ctx(device), buf, len(buf)), "fgmm_ctx_worker_cpus")
    return buf.value.decode()


def call_log(device: int, last: int = 64) -> list:
    """phase marks of the context's most recent batched calls, oldest first (include/flashgmm_amd.h: fgmm_ctx_call_log)"""
    buf = (fgmm_call_marks * 64)()
    n = C.c_int()
    check(lib().fgmm_ctx_call_log(ctx(device), buf, min(int(last), 64), C.byref(n)), "fgmm_ctx_call_log")
    return [{"kind": CALL_KINDS.get(m.kind, m.kind), "count": m.count, "t_begin_ms": m.t_begin_ms, "ms": list(m.ms),
             "worker_busy_ms": m.worker_busy_ms, "worker_wait_ms": m.worker_wait_ms, "head_ms": list(m.head_ms)} for m in buf[:n.value]]
