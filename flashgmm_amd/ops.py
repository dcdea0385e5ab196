"""Operators either side of the path.

``ckbd_unembed`` / ``ckbd_embed`` — ``CheckerboardLatentCodec.unembed / embed`` (compressai/latent_codecs/checkerboard.py:
333-377) as one HIP kernel each (the reference issues four strided slice assignments into a zero-filled tensor).

``CheckerboardContext`` — the checkerboard context convolution (a masked 5x5 ``CheckerboardMaskedConv2d(M, C_out)`` between an
``embed`` and an ``unembed``) as ONE HIP kernel on the matrix cores: compact anchors in, compact non-anchor context out, in one fixed
summation order (include/flashgmm_amd.h section 5b).

``pmf_to_quantized_cdf`` — mirror of ``compressai._CXX.pmf_to_quantized_cdf`` (compressai/cpp_exts/ops/ops.cpp:40-109),
the table builder behind ``EntropyBottleneck.update()`` / ``GaussianConditional.update()`` (the `z` hyper-latent path).
Runs once per model; host code in libflashgmm_amd.so."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib

__all__ = ["pmf_to_quantized_cdf", "ckbd_unembed", "ckbd_embed", "CheckerboardContext"]


def _ckbd(t, anchor_parity: str, embed: bool):
    import torch

    if anchor_parity not in ("even", "odd"):
        raise ValueError(f"anchor_parity {anchor_parity!r}")
    if not t.is_cuda:
        raise RuntimeError("flashgmm_amd operators run on the GPU only: the tensor must be on a HIP device")
    if t.element_size() not in (2, 4):
        raise RuntimeError(f"checkerboard split/merge handles 2- and 4-byte element types, got {t.dtype}")
    t = t.contiguous()
    if embed:
        if t.dim() != 5 or t.shape[0] != 2:
            raise RuntimeError(f"embed expects [2, n, c, h, w/2], got {tuple(t.shape)}")
        _, n, c, h, w2 = t.shape
        out = torch.empty((n, c, h, 2 * w2), dtype=t.dtype, device=t.device)
        fn, w = _lib.lib().fgmm_ckbd_embed, 2 * w2
    else:
        if t.dim() != 4:
            raise RuntimeError(f"unembed expects [n, c, h, w], got {tuple(t.shape)}")
        n, c, h, w = t.shape
        if w % 2:
            raise RuntimeError("unembed needs an even width (the reference's slicing does too)")
        out = torch.empty((2, n, c, h, w // 2), dtype=t.dtype, device=t.device)
        fn = _lib.lib().fgmm_ckbd_unembed
    dev = t.device.index if t.device.index is not None else -1
    rc = fn(_lib.ctx(dev), torch.cuda.current_stream(t.device).cuda_stream, t.data_ptr(), out.data_ptr(), n * c, h, w,
            t.element_size(), int(anchor_parity == "odd"))
    _lib.check(rc, "ckbd_embed" if embed else "ckbd_unembed")
    return out


def ckbd_unembed(y, anchor_parity: str = "even"):
    """``[n, c, h, w] -> [2, n, c, h, w/2]``: half 0 = anchors, half 1 = non-anchors (checkerboard.py:333-354)."""
    return _ckbd(y, anchor_parity, False)


def ckbd_embed(y_, anchor_parity: str = "even"):
    """``[2, n, c, h, w/2] -> [n, c, h, w]`` (checkerboard.py:356-377)."""
    return _ckbd(y_, anchor_parity, True)


class CheckerboardContext:
    """The context convolution of the checkerboard codec - ``unembed(context_prediction(embed([anchors, 0])))[1]`` with
    ``context_prediction`` a 5x5 ``CheckerboardMaskedConv2d(M, C_out, padding=2)`` (compressai/latent_codecs/checkerboard.py:281-284) -
    on the matrix cores in ONE fixed summation order (include/flashgmm_amd.h section 5b: bit for bit an ``fmaf`` chain over the 12 kept
    taps, row-major, and the input channels of each):

        ctx = CheckerboardContext(context_prediction, anchor_parity="even")   # an nn.Conv2d-like 5x5 module on the GPU
        y_ctx_1 = ctx.non_anchor(y_hat_[0])                                   # [N, M, h, w/2] -> [N, C_out, h, w/2]

    Only the 12 taps the mask keeps are multiplied, only at the non-anchor positions, and the non-anchor half of the input is never
    read.  Inference only: the weights are detached and packed once, here.  The result differs from MIOpen's convolution in its last
    bits, so encoder and decoder must both use it."""

    def __init__(self, conv, anchor_parity: str = "even"):
        import torch

        if anchor_parity not in ("even", "odd"):
            raise ValueError(f"anchor_parity {anchor_parity!r}")
        w = conv.weight.detach()
        def pair(v):
            return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

        if (w.dim() != 4 or tuple(w.shape[2:]) != (5, 5) or pair(getattr(conv, "stride", 1)) != (1, 1) or pair(getattr(conv, "padding", 2)) != (2, 2)
                or pair(getattr(conv, "dilation", 1)) != (1, 1) or getattr(conv, "groups", 1) != 1 or getattr(conv, "padding_mode", "zeros") != "zeros"):
            raise ValueError("expected a 5x5 convolution with stride 1, padding 2, dilation 1, groups 1 and zero padding")
        mask = getattr(conv, "mask", None)
        w = (w * mask if mask is not None else w).to(torch.float32).contiguous()
        dropped = w.reshape(w.shape[0], w.shape[1], 25)[:, :, 0::2]  # the kernel positions (i, j) with i + j even
        if bool((dropped != 0).any()) or bool(torch.isnan(dropped).any()):
            raise ValueError("a dropped tap (kernel position (i, j) with i + j even) of the effective weight is not zero: not a checkerboard-masked convolution")
        if not w.is_cuda:
            raise RuntimeError("flashgmm_amd operators run on the GPU only: the convolution's weights must be on a HIP device")
        self.anchor_parity = anchor_parity
        self.C_out, self.M = int(w.shape[0]), int(w.shape[1])
        self.device = w.device
        self._dev = w.device.index if w.device.index is not None else -1
        b = None if getattr(conv, "bias", None) is None else conv.bias.detach().to(torch.float32).contiguous()
        out = C.c_void_p()
        stream = torch.cuda.current_stream(w.device).cuda_stream
        _lib.check(_lib.lib().fgmm_ckbd_ctx_create(_lib.ctx(self._dev), stream, w.data_ptr(), b.data_ptr() if b is not None else None, self.M,
                                                   self.C_out, C.byref(out)), "CheckerboardContext")
        self._h = out

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().fgmm_ckbd_ctx_destroy(h)
            except Exception:  # pragma: no cover - interpreter shutdown
                pass

    def non_anchor(self, anchors):
        """``[N, M, h, w/2]`` float32, the anchors half (``unembed(.)[0]``) -> ``[N, C_out, h, w/2]``, the non-anchor half of the
        convolution's output (``unembed(.)[1]``).  Enqueued on the current stream; nothing waits."""
        import torch

        if anchors.dim() != 4 or anchors.shape[1] != self.M or anchors.device != self.device or anchors.dtype != torch.float32:
            raise RuntimeError(f"anchors must be float32 [N, {self.M}, h, w/2] on {self.device}; got {anchors.dtype} {tuple(anchors.shape)} on {anchors.device}")
        a = anchors.contiguous()
        N, _, h, w2 = a.shape
        out = torch.empty((N, self.C_out, h, w2), dtype=torch.float32, device=a.device)
        if N and h and w2:
            _lib.check(_lib.lib().fgmm_ckbd_ctx_apply(_lib.ctx(self._dev), torch.cuda.current_stream(a.device).cuda_stream, self._h, a.data_ptr(),
                                                      out.data_ptr(), N, h, 2 * w2, int(self.anchor_parity == "odd")), "CheckerboardContext.non_anchor")
        return out


def pmf_to_quantized_cdf(pmf: Sequence[float], precision: int = 16) -> List[int]:
    """Same contract as the reference: list of len(pmf)+1 ints, cdf[0] == 0, cdf[-1] == 1 << precision, strictly
    increasing; ``ValueError`` for negative / non-finite / all-zero input (pybind11 maps std::domain_error to it)."""
    a = np.ascontiguousarray(pmf, dtype=np.float32)
    if a.ndim != 1 or a.size == 0:
        raise ValueError("pmf must be a non-empty 1-D sequence")
    out = np.zeros(a.size + 1, np.uint32)
    rc = _lib.lib().fgmm_pmf_to_quantized_cdf(a.ctypes.data_as(C.c_void_p), a.size, int(precision),
                                               out.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("Invalid `pmf`: negative, non-finite or all-zero elements (or more symbols than counts)")
    return out.tolist()
