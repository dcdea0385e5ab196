"""Operators either side of the path.

``ckbd_unembed`` / ``ckbd_embed`` — ``CheckerboardLatentCodec.unembed / embed`` (compressai/latent_codecs/checkerboard.py:
333-377) as one HIP kernel each (the reference issues four strided slice assignments into a zero-filled tensor).

``CheckerboardContext`` — the checkerboard context convolution (a masked 5x5 ``CheckerboardMaskedConv2d(M, C_out)`` between an
``embed`` and an ``unembed``) as ONE HIP kernel on the matrix cores: compact anchors in, compact non-anchor context out, in one fixed
summation order (include/flashgmm_amd.h section 5b).

``checkerboard_context`` — the same convolution as a DIFFERENTIABLE operator (header section 5c): its data gradient is the forward kernel
over the transposed filters, its weight and bias gradients one matrix-core kernel in a summation order that is a function of the shape
alone.  ``ckbd_unembed`` / ``ckbd_embed`` are differentiable as well: each one's backward is the other.

``pmf_to_quantized_cdf`` — mirror of ``compressai._CXX.pmf_to_quantized_cdf`` (compressai/cpp_exts/ops/ops.cpp:40-109),
the table builder behind ``EntropyBottleneck.update()`` / ``GaussianConditional.update()`` (the `z` hyper-latent path).
Runs once per model; host code in libflashgmm_amd.so."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib

__all__ = ["pmf_to_quantized_cdf", "ckbd_unembed", "ckbd_embed", "CheckerboardContext", "checkerboard_context"]


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


_ckbd_fn = {}


def _ckbd_function(embed: bool):
    """the autograd form of the two permutations, made on first use (torch is imported lazily here): the backward of each is the
    other with the same parity"""
    if embed not in _ckbd_fn:
        import torch

        class _Ckbd(torch.autograd.Function):
            @staticmethod
            def forward(ctx, t, anchor_parity):
                ctx.anchor_parity = anchor_parity
                return _ckbd(t, anchor_parity, embed)

            @staticmethod
            @torch.autograd.function.once_differentiable
            def backward(ctx, grad):
                return _ckbd(grad, ctx.anchor_parity, not embed), None

        _Ckbd.__name__ = "CkbdEmbed" if embed else "CkbdUnembed"
        _ckbd_fn[embed] = _Ckbd
    return _ckbd_fn[embed]


def _ckbd_maybe_grad(t, anchor_parity: str, embed: bool):
    import torch

    if torch.is_tensor(t) and t.requires_grad and torch.is_grad_enabled():
        if anchor_parity not in ("even", "odd"):
            raise ValueError(f"anchor_parity {anchor_parity!r}")
        return _ckbd_function(embed).apply(t, anchor_parity)
    return _ckbd(t, anchor_parity, embed)


def ckbd_unembed(y, anchor_parity: str = "even"):
    """``[n, c, h, w] -> [2, n, c, h, w/2]``: half 0 = anchors, half 1 = non-anchors (checkerboard.py:333-354).  Differentiable: the
    backward is ``ckbd_embed`` of the gradient."""
    return _ckbd_maybe_grad(y, anchor_parity, False)


def ckbd_embed(y_, anchor_parity: str = "even"):
    """``[2, n, c, h, w/2] -> [n, c, h, w]`` (checkerboard.py:356-377).  Differentiable: the backward is ``ckbd_unembed`` of the
    gradient."""
    return _ckbd_maybe_grad(y_, anchor_parity, True)


class CheckerboardContext:
    """The context convolution of the checkerboard codec - ``unembed(context_prediction(embed([anchors, 0])))[1]`` with
    ``context_prediction`` a 5x5 ``CheckerboardMaskedConv2d(M, C_out, padding=2)`` (compressai/latent_codecs/checkerboard.py:281-284) -
    on the matrix cores in ONE fixed summation order (include/flashgmm_amd.h section 5b: bit for bit an ``fmaf`` chain over the 12 kept
    taps, row-major, and the input channels of each):

        ctx = CheckerboardContext(context_prediction, anchor_parity="even")   # an nn.Conv2d-like 5x5 module on the GPU
        y_ctx_1 = ctx.non_anchor(y_hat_[0])                                   # [N, M, h, w/2] -> [N, C_out, h, w/2]

    Only the 12 taps the mask keeps are multiplied, only at the non-anchor positions, and the non-anchor half of the input is never
    read.  Inference only: the weights are detached and packed once, here.  The result differs from MIOpen's convolution in its last
    bits, so encoder and decoder must both use it.

    Training: ``checkerboard_context(anchors, weight * mask, bias, anchor_parity)`` is the same operator under autograd (header section
    5c).  One documented difference from the reference: its ``CheckerboardMaskedConv2d`` zeroes ``weight.data`` in place and then
    differentiates a plain convolution (compressai/layers/layers.py:141-144), so its dropped taps receive non-zero gradients (which
    never change a forward value but enter a global gradient-norm clip); here the gradient is that of ``weight * mask``: +0 there."""

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


def _ctx_check(anchors, weight, bias, anchor_parity):
    """the refusals of ``checkerboard_context``: parity, device, dtype, shape (as ``CheckerboardContext.non_anchor``'s)"""
    import torch

    if anchor_parity not in ("even", "odd"):
        raise ValueError(f"anchor_parity {anchor_parity!r}")
    if not (torch.is_tensor(anchors) and torch.is_tensor(weight)) or (bias is not None and not torch.is_tensor(bias)):
        raise TypeError("anchors, weight and bias must be tensors")
    if weight.dim() != 4 or tuple(weight.shape[2:]) != (5, 5) or weight.dtype != torch.float32:
        raise RuntimeError(f"weight must be float32 [C_out, M, 5, 5]; got {weight.dtype} {tuple(weight.shape)}")
    C_out, M = int(weight.shape[0]), int(weight.shape[1])
    if not weight.is_cuda:
        raise RuntimeError("flashgmm_amd operators run on the GPU only: the convolution's weights must be on a HIP device")
    if anchors.dim() != 4 or anchors.shape[1] != M or anchors.device != weight.device or anchors.dtype != torch.float32:
        raise RuntimeError(f"anchors must be float32 [N, {M}, h, w/2] on {weight.device}; got {anchors.dtype} {tuple(anchors.shape)} on {anchors.device}")
    if bias is not None and (tuple(bias.shape) != (C_out,) or bias.device != weight.device or bias.dtype != torch.float32):
        raise RuntimeError(f"bias must be float32 [{C_out}] on {weight.device}; got {bias.dtype} {tuple(bias.shape)} on {bias.device}")
    return M, C_out


def _ctx_apply(dev, stream, w, b, transposed, M, C_out, x, odd):
    """pack (w [C_out, M, 5, 5], transposed or not) into a torch-allocated buffer and apply it to x on ``stream``: -> the output"""
    import torch

    L = _lib.lib()
    pm, pc = (C_out, M) if transposed else (M, C_out)  # the packed convolution's channel counts
    packed = torch.empty((int(L.fgmm_ckbd_ctx_packed_floats(pm, pc)),), dtype=torch.float32, device=x.device)
    _lib.check(L.fgmm_ckbd_ctx_pack(_lib.ctx(dev), stream, w.data_ptr(), b.data_ptr() if b is not None else None, M, C_out, int(transposed),
                                    packed.data_ptr()), "checkerboard_context: pack")
    N, _, h, w2 = x.shape
    out = torch.empty((N, pc, h, w2), dtype=torch.float32, device=x.device)
    if N and h and w2:
        _lib.check(L.fgmm_ckbd_ctx_apply_packed(_lib.ctx(dev), stream, packed.data_ptr(), pm, pc, x.data_ptr(), out.data_ptr(), N, h, 2 * w2, odd),
                   "checkerboard_context: apply")
    return out


_ctx_fn = []


def _ctx_function():
    if not _ctx_fn:
        import torch

        class CheckerboardContextFn(torch.autograd.Function):
            @staticmethod
            def forward(ctx, anchors, weight, bias, anchor_parity):
                M, C_out = _ctx_check(anchors, weight, bias, anchor_parity)
                a, w = anchors.detach().contiguous(), weight.detach().contiguous()
                b = None if bias is None else bias.detach().contiguous()
                dev = w.device.index if w.device.index is not None else -1
                odd = int(anchor_parity == "odd")
                out = _ctx_apply(dev, torch.cuda.current_stream(w.device).cuda_stream, w, b, False, M, C_out, a, odd)
                ctx.save_for_backward(a, w)
                ctx.odd, ctx.dev, ctx.has_bias = odd, dev, bias is not None
                return out

            @staticmethod
            @torch.autograd.function.once_differentiable
            def backward(ctx, g):
                a, w = ctx.saved_tensors
                C_out, M = int(w.shape[0]), int(w.shape[1])
                N, _, h, w2 = a.shape
                g = g.to(torch.float32).contiguous()
                stream = torch.cuda.current_stream(w.device).cuda_stream
                need_a, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
                da = dw = db = None
                if need_a:  # the forward operator on the output gradient: filters flipped and transposed, the other parity
                    da = _ctx_apply(ctx.dev, stream, w, None, True, M, C_out, g, ctx.odd ^ 1)
                if need_w or need_b:
                    L = _lib.lib()
                    dw = torch.empty_like(w) if need_w else None
                    db = torch.empty((C_out,), dtype=torch.float32, device=w.device) if need_b else None
                    if N and h and w2:
                        nbytes = int(L.fgmm_ckbd_ctx_wgrad_workspace(M, C_out, N, h, 2 * w2))
                        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=w.device)
                        _lib.check(L.fgmm_ckbd_ctx_wgrad(_lib.ctx(ctx.dev), stream, a.data_ptr(), g.data_ptr(), M, C_out, N, h, 2 * w2, ctx.odd,
                                                         dw.data_ptr() if need_w else None, db.data_ptr() if need_b else None, ws.data_ptr(), nbytes),
                                   "checkerboard_context: wgrad")
                    else:  # an empty sum
                        dw = dw.zero_() if need_w else None
                        db = db.zero_() if need_b else None
                return da, dw, db, None

        _ctx_fn.append(CheckerboardContextFn)
    return _ctx_fn[0]


def checkerboard_context(anchors, weight, bias=None, anchor_parity: str = "even"):
    """``CheckerboardContext.non_anchor`` as a differentiable operator (include/flashgmm_amd.h sections 5b and 5c): ``anchors``
    ``[N, M, h, w/2]`` float32 (``ckbd_unembed(y_hat)[0]``), ``weight`` the EFFECTIVE ``[C_out, M, 5, 5]`` float32 weight - pass
    ``conv.weight * conv.mask``, so that autograd applies the mask to the gradient; the dropped taps are not looked at - and ``bias``
    ``[C_out]`` or None -> ``[N, C_out, h, w/2]``, the non-anchor half of the convolution's output, bit for bit section 5b's chain.
    The weights are packed at every call (a training step changes them), into torch-allocated memory on the current stream.

    Backward (once differentiable, only what is asked for): the gradient of ``anchors`` is the forward kernel on the transposed,
    flipped filters with the other parity; those of ``weight`` and ``bias`` one matrix-core kernel over a torch-allocated workspace,
    in a summation order that depends on the shape alone - the same bits on every run, device and launch geometry.  The gradient of
    ``weight`` is +0 at the 13 dropped taps of every filter: that of ``weight * mask``, where the reference - which zeroes
    ``weight.data`` in place and differentiates a plain convolution (compressai/layers/layers.py:141-144) - leaves non-zero values
    that never change a forward value but do enter a global gradient-norm clip."""
    _ctx_check(anchors, weight, bias, anchor_parity)
    return _ctx_function().apply(anchors, weight, bias, anchor_parity)


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
