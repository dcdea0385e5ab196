"""``GaussianMixtureConditionalLatentCodec`` — the caller right above the path, same compress/decompress contract as
the reference's (compressai/latent_codecs/gaussian_mixture_conditional.py:43-202), built on
``flashgmm_amd.GaussianMixtureConditional``:

    codec.compress(y, ctx_params)             -> {"strings": [(bytes, abs_max, zero_bitmap)], "shape": (h, w), "y_hat": y_q}
    codec.decompress(strings, shape, ctx_params) -> {"y_hat": y_hat}

``entropy_parameters(ctx_params)`` yields ``[1, 3*K*M, h, w]``; it is split with ``chunk(3, 1)`` into scales, means and
mixture logits, the logits are soft-maxed over K on the ``[1, K, M, h, w]`` view (:183-202) — all views / stock torch ops
on the GPU — and handed to the entropy model in place.  Both quantizers of the reference are kept ("noise": code round(y);
"weighted_mean_ste": code round(y - sum_k pi_k mu_k) against re-centred means, :135-145, :167-179).
``forward`` (:99-125) returns the differentiable likelihoods and ``y_hat`` from ``GaussianMixtureConditional.forward``, the fused
likelihood kernel; the checkerboard, channel-group and hyper codecs below keep their ``forward`` stubs.

``CheckerboardLatentCodec`` and ``ChannelGroupsLatentCodec`` mirror the two codecs that drive the path in the
reference's GMM models (compressai/latent_codecs/checkerboard.py:275-330, channel_groups.py:111-158;
models/ckbd_gmm.py:111, models/elic_gmm.py:198-219): same constructor arguments, same ``compress / decompress``
contract and nested ``{"strings": [...], "shape": ...}`` result, the networks (``context_prediction``,
``entropy_parameters``, ``channel_context``) supplied by the caller as torch modules.  What changes is the schedule:
the checkerboard split / merge is one HIP kernel each, and on encode both halves are coded in ONE batched call —
the anchors' reconstruction that the non-anchor parameters depend on is ``round(.)`` of data the encoder already
holds (checkerboard.py:282-288), so nothing has to wait for the anchors' bitstream.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch import Tensor

from itertools import accumulate

from .entropy_models import EntropyBottleneck, EntropyBottleneckCoder, GaussianMixtureConditional, ParameterHead
from .ops import CheckerboardContext, checkerboard_context, ckbd_embed, ckbd_unembed

__all__ = ["GaussianMixtureConditionalLatentCodec", "CheckerboardLatentCodec", "ChannelGroupsLatentCodec", "HyperLatentCodec",
           "HyperpriorLatentCodec"]


def _check_rdo_lambda(lam) -> float:
    lam = float(lam)
    if not (0.0 <= lam < float("inf")):
        raise ValueError(f"rdo_lambda = {lam!r}: must be finite and >= 0")
    return lam


def _check_target_bytes(n) -> Optional[int]:
    if n is None:
        return None
    if int(n) != n or int(n) < 0:
        raise ValueError(f"target_bytes = {n!r}: must be an integer >= 0")
    return int(n)


class GaussianMixtureConditionalLatentCodec(nn.Module):
    def __init__(self, K: int = 4, gaussian_mixture_conditional: Optional[GaussianMixtureConditional] = None,
                 entropy_parameters: Optional[nn.Module] = None, quantizer: str = "noise",
                 chunks: Tuple[str, ...] = ("scales", "means", "weights"), mode=None, param_dtype: torch.dtype = torch.float32,
                 fuse_softmax: bool = False, checkpoint_stride: int = 0, rdo_lambda: float = 0.0, target_bytes: Optional[int] = None,
                 rdo_channel_weights: Optional[Tensor] = None, rdo_channel_skip: bool = False, fuse_forward_softmax: bool = False,
                 centroid: bool = False, centroid_p_min: float = 2.0 ** -16, **kwargs: Any):
        super().__init__()
        # centroid: the decompress calls add "y_rec" beside "y_hat" - per latent the conditional mean of its bin under the mixture it was
        # decoded with (GaussianMixtureConditional.reconstruct, include/flashgmm_amd.h section 3i), which minimises the expected squared
        # LATENT error; what that buys in the image domain depends on the trained synthesis transform and has not been measured.  A
        # decoder-side choice: "y_hat" and the bitstreams are untouched, the encoder needs no switch.  False: no new key, nothing launched
        self.centroid = bool(centroid)
        self.centroid_p_min = float(centroid_p_min)
        if not 0.0 < self.centroid_p_min < float("inf"):
            raise ValueError("centroid_p_min must be positive and finite")
        # fuse_forward_softmax: forward() hands the parameter network's output to GaussianMixtureConditional.forward_params as it is -
        # the softmax over K and its derivative run inside the two likelihood kernels (include/flashgmm_amd.h section 3h), on the pi
        # the coder's kernels make of the same logits, and the gradient of the output is written as one tensor.  It does not touch
        # the coding path (fuse_softmax is that path's switch)
        if fuse_forward_softmax and quantizer != "noise":
            raise ValueError("fuse_forward_softmax needs quantizer='noise' (the re-centring quantizer uses pi itself)")
        self.fuse_forward_softmax = bool(fuse_forward_softmax)
        # rdo_channel_skip: the two quantisations below may also drop a coded channel whole where that lowers distortion + lambda * bits
        # (include/flashgmm_amd.h section 3f).  It has an effect only together with rdo_lambda > 0 or target_bytes
        self.rdo_channel_skip = bool(rdo_channel_skip)
        # rdo_channel_weights: a float32 [M] buffer of per-channel factors of the squared error in the two quantisations below
        # (include/flashgmm_amd.h section 3e: the latent-domain proxy for what a step in that channel costs the image), every factor in
        # [0, 256].  With rdo_lambda == 0 and no target_bytes it does nothing and costs no launch
        if rdo_channel_weights is not None:
            rdo_channel_weights = torch.as_tensor(rdo_channel_weights)
            if rdo_channel_weights.dtype != torch.float32 or rdo_channel_weights.dim() != 1:
                raise ValueError("rdo_channel_weights must be a float32 tensor of shape [M]")
            rdo_channel_weights = rdo_channel_weights.detach().clone()
        self.register_buffer("rdo_channel_weights", rdo_channel_weights)
        # rdo_lambda > 0: rate-distortion optimised quantisation (GaussianMixtureConditional.quantize_rdo) - what is coded is, per latent,
        # round(.) or one of its two neighbours, whichever minimises (y - v)^2 + rdo_lambda * bits(v).  An encoder-side choice: the
        # decoder needs no switch.  0: plain rounding, no extra launch
        self.rdo_lambda = _check_rdo_lambda(rdo_lambda)
        # target_bytes: quantisation to a byte budget (GaussianMixtureConditional.quantize_to_budget) - the lambda of the above is
        # searched so that the PREDICTED length of the bitstream is at most this many bytes (a real stream may be 4 bytes longer, see
        # RateEstimate.nbytes; if no lambda up to the search's lambda_max fits, the result at lambda_max is coded).  Either a lambda or
        # a budget, not both
        self.target_bytes = _check_target_bytes(target_bytes)
        if self.target_bytes is not None and self.rdo_lambda > 0:
            raise ValueError("target_bytes together with rdo_lambda > 0: give either the lambda or the budget that determines it")
        if param_dtype not in (torch.float32, torch.float16, torch.bfloat16):
            raise ValueError("param_dtype must be torch.float32, torch.float16 or torch.bfloat16")
        # float16: BASELINE configs[4], "fp16 (mu, sigma, pi) with fp32 CDF accumulate"; bfloat16: the same bytes with float32's range
        self.param_dtype = param_dtype
        # fuse_softmax: the softmax over K (:198-202) runs inside the HIP kernels, on the head's logits in place — the pi
        # plane (16 B / latent written, 16 read back) never exists.  One fixed fp32 sequence on both sides of the codec:
        # streams are self-consistent on any device; they are NOT the streams of the un-fused path (torch.softmax's pi
        # differs in the last bit), so encoder and decoder must agree on this switch like on the Phi approximation.
        if fuse_softmax and (quantizer != "noise" or param_dtype != torch.float32):
            raise ValueError("fuse_softmax needs quantizer='noise' (the re-centring quantizer uses pi itself) and float32 planes")
        self.fuse_softmax = bool(fuse_softmax)
        if quantizer not in ("noise", "weighted_mean_ste"):
            raise ValueError(f"quantizer {quantizer} not supported")
        if tuple(chunks) != ("scales", "means", "weights"):
            raise ValueError("a Gaussian-mixture codec needs chunks = ('scales', 'means', 'weights')")
        self.K = K
        self.quantizer = quantizer
        # checkpoint_stride > 0: the strings are CheckpointedBytes — the same bitstreams plus out-of-band notes of the coder
        # state every that many symbols, with which ONE bitstream decodes on all host workers (a single image: 3.7 -> 1.6 ms
        # on a Kodak image, 108 -> 25 ms on a 4K ELIC image); flashgmm_amd.container stores them with the stream
        self.gaussian_mixture_conditional = gaussian_mixture_conditional or GaussianMixtureConditional(
            K=K, mode=mode, checkpoint_stride=checkpoint_stride)
        self.entropy_parameters = entropy_parameters or nn.Identity()
        self.chunks = tuple(chunks)

    # :183-196
    def _chunk(self, params: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
        scales, means, weights = params.chunk(3, 1)
        return scales, means, weights

    # :198-202
    def _reshape_gmm_weight(self, weight: Tensor) -> Tensor:
        B, KM, H, W = weight.shape
        weight = torch.reshape(weight, (B, self.K, KM // self.K, H, W))
        weight = nn.functional.softmax(weight, dim=1)
        return torch.reshape(weight, (B, KM, H, W))

    def _params(self, ctx_params: Tensor):
        scales_hat, means_hat, weights = self._chunk(self.entropy_parameters(ctx_params))
        return scales_hat, means_hat, (weights if self.fuse_softmax else self._reshape_gmm_weight(weights))

    def _planes(self, scales: Tensor, means: Tensor, weights: Tensor):
        """the planes as the entropy model gets them: float32 as they are, or float16 / bfloat16 copies — weights rounded TOWARD ZERO,
        because the algorithm needs sum_k pi_k <= 1 after widening (tests/synth.py to_float16_planes does it for the synthetic workloads);
        scales and means rounded to nearest"""
        if self.param_dtype == torch.float32:
            return scales, means, weights
        if self.param_dtype == torch.bfloat16:
            # toward zero = the low 16 bits of the binary32 pattern cleared; the conversion of what is left is exact
            wz = (weights.contiguous().view(torch.int32) & -65536).view(torch.float32)
            return scales.to(torch.bfloat16), means.to(torch.bfloat16), wz.to(torch.bfloat16)
        w16 = weights.to(torch.float16)
        over = w16.to(torch.float32) > weights
        w16 = torch.where(over, torch.nextafter(w16, torch.zeros_like(w16)), w16)
        return scales.to(torch.float16), means.to(torch.float16), w16

    def _recentre(self, means_hat: Tensor, weights: Tensor):
        """weighted_mean_ste: sum_k pi_k mu_k and the means relative to it (:139-144)"""
        B, KM, H, W = means_hat.shape
        me = means_hat.view(B, self.K, KM // self.K, H, W)
        we = weights.view(B, self.K, KM // self.K, H, W)
        weighted_sum = torch.sum(me * we, dim=1)
        return weighted_sum, (me - weighted_sum.unsqueeze(1)).reshape(B, KM, H, W)

    def _rdo(self, y_code: Tensor, planes, lam: float, position_weights: Optional[Tensor] = None, channel_skip: Optional[bool] = None):
        """(y_to_code, planes) with y_to_code replaced by its rate-distortion optimised quantisation (integer-valued: the encode path
        then rounds it to itself)"""
        q = self.gaussian_mixture_conditional.quantize_rdo(y_code, *planes, lam, weights_are_logits=self.fuse_softmax,
                                                           channel_weights=self.rdo_channel_weights, position_weights=position_weights,
                                                           channel_skip=self.rdo_channel_skip if channel_skip is None else bool(channel_skip))
        return (q.y, *planes)

    def coder_inputs(self, y: Tensor, ctx_params: Tensor, position_weights: Optional[Tensor] = None):
        """What ``compress`` hands the entropy model: ``(y_to_code, scales, means, weights)``.  ``round(y_to_code)`` is
        the ``y_hat`` that ``compress`` returns (:127-149) — known before any coding happens.  With the codec's ``rdo_lambda`` > 0
        ``y_to_code`` is the RDOQ result of what would be rounded; with its ``target_bytes`` set, the RDOQ result at the lambda that
        budget determines."""
        if self.target_bytes is not None:
            return self.coder_inputs_budget(y, ctx_params, self.target_bytes, position_weights)
        return self.coder_inputs_rdo(y, ctx_params, self.rdo_lambda, position_weights)

    def coder_inputs_budget(self, y: Tensor, ctx_params: Tensor, budget_bytes: int, position_weights: Optional[Tensor] = None):
        """``coder_inputs`` with what would be rounded quantised to ``budget_bytes`` of predicted bitstream
        (``GaussianMixtureConditional.quantize_to_budget``, its default search).  ``position_weights`` (``[h, w]`` or ``[1, 1, h, w]``)
        and the codec's ``rdo_channel_weights`` weight the squared error (section 3e)"""
        budget = _check_target_bytes(budget_bytes)
        if budget is None:
            raise ValueError("budget_bytes must be given")
        scales_hat, means_hat, weights = self._params(ctx_params)
        y_code = y
        if self.quantizer != "noise":
            weighted_sum, means_hat = self._recentre(means_hat, weights)
            y_code = y - weighted_sum
        planes = self._planes(scales_hat, means_hat, weights)
        q = self.gaussian_mixture_conditional.quantize_to_budget(y_code, *planes, budget, weights_are_logits=self.fuse_softmax,
                                                                 channel_weights=self.rdo_channel_weights, position_weights=position_weights,
                                                                 channel_skip=self.rdo_channel_skip)
        return (q.y, *planes)

    def coder_inputs_rdo(self, y: Tensor, ctx_params: Tensor, rdo_lambda: float, position_weights: Optional[Tensor] = None,
                         channel_skip: Optional[bool] = None):
        """``coder_inputs`` with a given ``rdo_lambda`` in place of the codec's own (0: plain rounding, no extra launch - weights then do
        nothing).  ``position_weights``: as ``coder_inputs_budget`` takes it.  ``channel_skip``: in place of the codec's own
        ``rdo_channel_skip`` (None: the codec's)"""
        lam = _check_rdo_lambda(rdo_lambda)
        scales_hat, means_hat, weights = self._params(ctx_params)
        if self.quantizer == "noise":
            planes = self._planes(scales_hat, means_hat, weights)
            return self._rdo(y, planes, lam, position_weights, channel_skip) if lam > 0 else (y, *planes)
        weighted_sum, means_rel = self._recentre(means_hat, weights)
        d = y - weighted_sum
        if lam > 0:
            return self._rdo(d, self._planes(scales_hat, means_rel, weights), lam, position_weights, channel_skip)
        # quantize_ste (compressai/ops/ops.py:66-80) is (round(d) - d) + d: the value of round(d), but +0.0 where
        # round(d) is -0.0 — kept, so that the returned y_hat has the reference's bits
        return ((torch.round(d) - d) + d, *self._planes(scales_hat, means_rel, weights))

    def compress(self, y: Tensor, ctx_params: Tensor) -> Dict[str, Any]:
        y_code, scales_hat, means_hat, weights = self.coder_inputs(y, ctx_params)
        y_strings, y_hat = self.gaussian_mixture_conditional.compress(y_code, scales_hat, means_hat, weights,
                                                                      weights_are_logits=self.fuse_softmax)
        return {"strings": [y_strings], "shape": y.shape[2:4], "y_hat": y_hat}

    def compress_many(self, prepared: List[Tuple[Tensor, Tensor, Tensor, Tensor]]) -> List[Dict[str, Any]]:
        """``compress`` of several ``coder_inputs`` results in one batched native call."""
        ys, ss, ms, ws = zip(*prepared)
        res = self.gaussian_mixture_conditional.compress_batch(list(ys), list(ss), list(ms), list(ws), weights_are_logits=self.fuse_softmax)
        return [{"strings": [(b, a, zb.to(y.device))], "shape": y.shape[2:4], "y_hat": yq}
                for ((b, a, zb), yq), y in zip(res, ys)]

    def estimate_many(self, prepared: List[Tuple[Tensor, Tensor, Tensor, Tensor]], **kwargs: Any):
        """the sizes of what ``compress_many`` would return for the same ``coder_inputs`` results, without coding them: a list of
        ``RateEstimate`` (``GaussianMixtureConditional.estimate_bits_batch``; ``per_channel`` / ``per_latent`` are passed on)"""
        ys, ss, ms, ws = zip(*prepared)
        return self.gaussian_mixture_conditional.estimate_bits_batch(list(ys), list(ss), list(ms), list(ws), weights_are_logits=self.fuse_softmax, **kwargs)

    def decompress(self, strings: List[Any], shape: Tuple[int, int], ctx_params: Tensor, **kwargs: Any) -> Dict[str, Any]:
        (y_strings,) = strings
        scales_hat, means_hat, weights = self._params(ctx_params)
        weighted_sum = None
        if self.quantizer == "noise":
            planes = self._planes(scales_hat, means_hat, weights)
            decoded = self.gaussian_mixture_conditional.decompress(*y_strings, *planes, weights_are_logits=self.fuse_softmax)
            y_hat = decoded
        else:
            weighted_sum, means_rel = self._recentre(means_hat, weights)
            planes = self._planes(scales_hat, means_rel, weights)
            decoded = self.gaussian_mixture_conditional.decompress(*y_strings, *planes)
            y_hat = decoded + weighted_sum
        assert tuple(y_hat.shape[2:4]) == tuple(shape)
        if not self.centroid:
            return {"y_hat": y_hat}
        return {"y_hat": y_hat, "y_rec": self._reconstruct([decoded], [planes], [weighted_sum], self.fuse_softmax)[0]}

    def _reconstruct(self, decoded: List[Tensor], planes, sums, logits: bool) -> List[Tensor]:
        """The "y_rec" of decoded items: the centroid of what the coder decoded, under the planes the coder was given (one batched call);
        for ``weighted_mean_ste`` that is the residual under the relative means, and ``weighted_sum`` is added afterwards"""
        ss, ms, ws = (list(t) for t in zip(*planes))
        recs = self.gaussian_mixture_conditional.reconstruct_batch(decoded, ss, ms, ws, weights_are_logits=logits, p_min=self.centroid_p_min)
        return [rec if add is None else rec + add for rec, add in zip(recs, sums)]

    # ---- the parameter head fused: `feat` = the input of entropy_parameters' LAST layer, `head` = a ParameterHead
    # of that layer.  The codec owning the parameter network (CheckerboardLatentCodec(fuse_head=True)) calls these.
    def _check_head(self):
        if self.quantizer != "noise" or self.param_dtype != torch.float32:
            raise RuntimeError("the fused parameter head needs quantizer='noise' and float32 parameters (as fuse_softmax)")

    def compress_many_head(self, items: List[Tuple[Tensor, Tensor]], head: ParameterHead) -> List[Dict[str, Any]]:
        """``compress`` of several ``(y [1, M, h, w], feat [1, c_in, h, w])`` of one shape in ONE native call, the parameters computed
        by the head inside the encode-side kernel (never written to HBM)"""
        self._check_head()
        ys, feats = zip(*items)
        res = self.gaussian_mixture_conditional.compress_head_batch(torch.cat(list(ys)), torch.cat(list(feats)), head)
        return [{"strings": [(b, a, zb.to(y.device))], "shape": y.shape[2:4], "y_hat": yq} for ((b, a, zb), yq), y in zip(res, ys)]

    def decompress_many_head(self, strings: List[List[Any]], shape: Tuple[int, int], feats: List[Tensor], head: ParameterHead) -> List[Dict[str, Any]]:
        """the decoder's side: the SAME arithmetic gives the parameter tensors (``head.params``), the table kernels take the logits"""
        self._check_head()
        scales, means, logits = head.params(torch.cat(list(feats)))
        items = [st[0] for st in strings]
        outs = self.gaussian_mixture_conditional.decompress_batch([it[0] for it in items], [it[1] for it in items],
                                                                  torch.stack([it[2].to("cpu", torch.int64) for it in items]), scales, means, logits,
                                                                  weights_are_logits=True)
        for y_hat in outs:
            assert tuple(y_hat.shape[2:4]) == tuple(shape)
        if not self.centroid:
            return [{"y_hat": y_hat} for y_hat in outs]
        recs = self.gaussian_mixture_conditional.reconstruct_batch(torch.cat(list(outs)), scales, means, logits, weights_are_logits=True,
                                                                   p_min=self.centroid_p_min)  # (under the head's logits, as decoded)
        return [{"y_hat": y_hat, "y_rec": rec} for y_hat, rec in zip(outs, recs)]

    def decompress_many(self, strings: List[List[Any]], shape: Tuple[int, int], ctx_params: List[Tensor]) -> List[Dict[str, Any]]:
        """``decompress`` of N independent items (the same stage of N images) in ONE batched native call: N host decoders
        side by side instead of N calls with one decoder each."""
        planes, sums = [], []
        for ctx in ctx_params:
            scales_hat, means_hat, weights = self._params(ctx)
            if self.quantizer == "noise":
                planes.append(self._planes(scales_hat, means_hat, weights))
                sums.append(None)
            else:
                weighted_sum, means_rel = self._recentre(means_hat, weights)
                planes.append(self._planes(scales_hat, means_rel, weights))
                sums.append(weighted_sum)
        items = [st[0] for st in strings]  # (bytes, abs_max, zero_bitmap) of every item
        ss, ms, ws = (list(t) for t in zip(*planes))
        outs = self.gaussian_mixture_conditional.decompress_batch([it[0] for it in items], [it[1] for it in items], [it[2] for it in items],
                                                                  ss, ms, ws, weights_are_logits=self.fuse_softmax)
        res = []
        for y_hat, add in zip(outs, sums):
            assert tuple(y_hat.shape[2:4]) == tuple(shape)
            res.append({"y_hat": y_hat if add is None else y_hat + add})
        if self.centroid:
            for r, rec in zip(res, self._reconstruct(list(outs), planes, sums, self.fuse_softmax)):
                r["y_rec"] = rec
        return res

    def forward(self, y: Tensor, ctx_params: Tensor) -> Dict[str, Any]:
        """As the reference's (latent_codecs/gaussian_mixture_conditional.py:99-125): ``{"likelihoods": {"y": ...}, "y_hat": ...}``
        from ``GaussianMixtureConditional.forward`` (the fused likelihood kernel, differentiable), for both quantizers.  The planes
        are the parameter network's as they are, the weights torch's softmax over K (autograd differentiates both): ``param_dtype``
        and ``fuse_softmax`` are choices of the coding path and do not apply here.  With ``fuse_forward_softmax`` the softmax over K
        runs in the likelihood kernels instead: ``GaussianMixtureConditional.forward_params`` on the parameter network's output."""
        if self.fuse_forward_softmax:
            y_hat, y_likelihoods = self.gaussian_mixture_conditional.forward_params(y, self.entropy_parameters(ctx_params))
            return {"likelihoods": {"y": y_likelihoods}, "y_hat": y_hat}
        scales_hat, means_hat, weights = self._chunk(self.entropy_parameters(ctx_params))
        weights = self._reshape_gmm_weight(weights)
        if self.quantizer == "noise":
            y_hat, y_likelihoods = self.gaussian_mixture_conditional(y, scales_hat, means_hat, weights)
        else:
            weighted_sum, means_hat = self._recentre(means_hat, weights)
            d = y - weighted_sum
            y_hat = ((torch.round(d) - d).detach() + d) + weighted_sum  # quantize_ste (compressai/ops/ops.py:66-80)
            y_hat, y_likelihoods = self.gaussian_mixture_conditional(y_hat, scales_hat, means_hat, weights)
        return {"likelihoods": {"y": y_likelihoods}, "y_hat": y_hat}


class CheckerboardLatentCodec(nn.Module):
    """Two-pass checkerboard context model: ``compress`` / ``decompress`` (checkerboard.py:275-330), and the one-pass training
    ``forward`` (checkerboard.py:154-171).

    ``latent_codec["y"]`` is a ``GaussianMixtureConditionalLatentCodec`` (its own ``entropy_parameters`` is the
    identity: the parameter network sits here, as in the reference's models); ``entropy_parameters`` must be
    pointwise (the reference's warning, checkerboard.py:80-82); batch size 1 (checkerboard.py:307)."""

    def __init__(self, latent_codec: Optional[Dict[str, nn.Module]] = None, entropy_parameters: Optional[nn.Module] = None,
                 context_prediction: Optional[nn.Module] = None, anchor_parity: str = "even", forward_method: str = "twopass",
                 fuse_head=False, rdo_lambda: float = 0.0, rdo_channel_skip: bool = False, fuse_context: bool = False, **kwargs: Any):
        super().__init__()
        # fuse_context: context_prediction - a 5x5 CheckerboardMaskedConv2d(M, C_out, padding=2) - runs inside the library
        # (flashgmm_amd.ops.CheckerboardContext, header section 5b: compact anchors in, compact non-anchor context out, one launch on the
        # matrix cores in ONE fixed summation order; the anchors' context is zeros and costs no convolution).  Like fuse_softmax and
        # fuse_head it changes the last bits of the parameters: the streams are self-consistent on any ROCm / MIOpen version, but they are
        # not the un-fused path's streams - encoder and decoder must agree on this switch.  Works alone and together with fuse_head.
        # In compress / decompress the weights are detached; forward() runs the same operator under autograd (section 5c).
        self.fuse_context = bool(fuse_context)
        self._context: Optional[CheckerboardContext] = None
        self._context_key = None
        # rdo_channel_skip: channel skipping (section 3f) in the halves' quantisation at THIS codec's rdo_lambda - with rdo_lambda > 0 it
        # replaces the inner codec's setting, as the lambda does; with rdo_lambda == 0 the inner codec's own settings apply
        self.rdo_channel_skip = bool(rdo_channel_skip)
        # rdo_lambda > 0: each half's latents are quantised with rate-distortion optimisation before the half's y_hat is taken, so the
        # non-anchors' context sees what the decoder will see (prepare); 0: the latent codec's own setting.  Precedence when both
        # this codec and its latent codec "y" carry an rdo_lambda: this one, if > 0, REPLACES the inner codec's for both halves (the two
        # are never combined); only when this one is 0 does the inner codec's own rdo_lambda apply
        # (No byte budget here: the non-anchor half's parameters depend on the anchor half's y_hat, so ONE lambda for both halves that
        # meets a budget on their sum needs the context network inside the search loop - a search over whole compress passes, not over
        # the curve of section 3d.  A latent codec "y" built with target_bytes still budgets each half on its own.)
        self.rdo_lambda = _check_rdo_lambda(rdo_lambda)
        if fuse_head and self.rdo_lambda > 0:
            raise RuntimeError("rdo_lambda > 0 together with fuse_head is not supported: RDOQ needs the parameter planes the fused head never writes")
        if anchor_parity not in ("even", "odd"):
            raise ValueError(f"anchor_parity {anchor_parity!r}")
        # fuse_head: the LAST layer of entropy_parameters - nn.Conv2d(c_in, 3*K*M, 1), models/ckbd_gmm.py:115-121 - runs inside the
        # library (flashgmm_amd.ParameterHead: matrix cores, one fixed summation order, fused with the encode-side CDF kernel; the
        # softmax over K and the sigma clamp with it): encoder and decoder must agree on this switch like on the Phi approximation -
        # the parameters differ from torch's convolution in their last bits
        # fuse_head: True / "f32" (the exact form) or "bf16x6" (ParameterHead's faster arithmetic: MI355X on both sides)
        if fuse_head not in (False, True, "f32", "bf16x6"):
            raise ValueError(f"fuse_head {fuse_head!r}")
        self.fuse_head = bool(fuse_head)
        self._head_arith = "bf16x6" if fuse_head == "bf16x6" else "f32"
        self._head: Optional[ParameterHead] = None
        self._head_key = None
        if self.fuse_head:
            last = entropy_parameters[-1] if isinstance(entropy_parameters, nn.Sequential) and len(entropy_parameters) else entropy_parameters
            if not isinstance(last, nn.Conv2d) or last.kernel_size != (1, 1) or last.stride != (1, 1) or last.groups != 1:
                raise ValueError("fuse_head needs entropy_parameters to end in a plain 1x1 nn.Conv2d (models/ckbd_gmm.py:115-121)")
        self.anchor_parity = anchor_parity
        self.non_anchor_parity = {"odd": "even", "even": "odd"}[anchor_parity]
        self.forward_method = forward_method
        self.entropy_parameters = entropy_parameters or nn.Identity()
        self.context_prediction = context_prediction or nn.Identity()
        self.latent_codec = nn.ModuleDict(latent_codec if latent_codec is not None
                                          else {"y": GaussianMixtureConditionalLatentCodec()})
        if self.fuse_head and getattr(self.latent_codec["y"], "rdo_channel_weights", None) is not None:
            raise RuntimeError("rdo_channel_weights together with fuse_head is not supported: RDOQ needs the parameter planes the fused head never writes")

    def __getitem__(self, key: str) -> nn.Module:
        return self.latent_codec[key]

    # checkerboard.py:333-377, one kernel each
    def unembed(self, y: Tensor) -> Tensor:
        return ckbd_unembed(y, self.anchor_parity)

    def embed(self, y_: Tensor) -> Tensor:
        return ckbd_embed(y_, self.anchor_parity)

    def merge(self, *args: Tensor) -> Tensor:
        return torch.cat(args, dim=1)

    def _head_parts(self):
        """-> (everything of entropy_parameters before its last layer, the ParameterHead of that layer): packed once, again when the
        layer's weights have changed (a checkpoint loaded, a device move)"""
        ep = self.entropy_parameters
        body, last = (ep[:-1], ep[-1]) if isinstance(ep, nn.Sequential) else (nn.Identity(), ep)
        key = (last.weight.data_ptr(), last.weight._version, None if last.bias is None else (last.bias.data_ptr(), last.bias._version))
        if self._head is None or self._head_key != key:
            self._head, self._head_key = ParameterHead(last, K=self.latent_codec["y"].K, arithmetic=self._head_arith), key
        return body, self._head

    def _context_op(self) -> CheckerboardContext:
        """the CheckerboardContext of context_prediction: packed once, again when its weights have changed (the key of _head_parts)"""
        cp = self.context_prediction
        bias = getattr(cp, "bias", None)
        key = (cp.weight.data_ptr(), cp.weight._version, None if bias is None else (bias.data_ptr(), bias._version))
        if self._context is None or self._context_key != key:
            self._context, self._context_key = CheckerboardContext(cp, self.anchor_parity), key
        return self._context

    def _ctx(self, y_hat_: Tensor, i: int) -> Tensor:
        """context of half i from the halves reconstructed so far (:281-284, :310-313)"""
        if self.fuse_context:
            op = self._context_op()
            if i == 0:  # _mask(., "all") for the anchors: no convolution runs for them
                return y_hat_.new_zeros((y_hat_.shape[1], op.C_out) + tuple(y_hat_.shape[3:]))
            return op.non_anchor(y_hat_[0])
        y_ctx_i = self.unembed(self.context_prediction(self.embed(y_hat_)))[i]
        return torch.zeros_like(y_ctx_i) if i == 0 else y_ctx_i  # _mask(., "all") for the anchors

    def prepare(self, y: Tensor, side_params: Tensor, importance: Optional[Tensor] = None):
        """Everything of ``compress`` that is not coding: -> (coder inputs of the two halves, y_hat).  The reconstruction
        a half's parameters depend on is ``round(.)`` of data the encoder holds (checkerboard.py:282-288), so the coder
        inputs of BOTH halves — and ``y_hat`` — exist before a single symbol is coded.  ``importance``: a float32 ``[1, 1, h, w]``
        map of per-position factors of the squared error in the halves' rate-distortion optimised quantisation (section 3e: region
        of interest, perceptual masking), every factor in [0, 256]; it is split as the latent is and half i's part handed to half i.
        Where no half is quantised that way (no rdo_lambda, no target_bytes) it does nothing and costs no launch."""
        n, c, h, w = y.shape
        if n != 1:
            raise RuntimeError("batch size 1 (as the reference's coder path, checkerboard.py:307)")
        codec = self.latent_codec["y"]
        if importance is not None:
            if self.fuse_head:
                raise RuntimeError("importance together with fuse_head is not supported: RDOQ needs the parameter planes the fused head never writes")
            if not isinstance(importance, Tensor) or importance.dtype != torch.float32:
                raise TypeError("importance must be a float32 tensor")
            if tuple(importance.shape) != (1, 1, h, w):
                raise ValueError(f"importance: shape {tuple(importance.shape)}, expected {(1, 1, h, w)}")
        rdo_runs = self.rdo_lambda > 0 or getattr(codec, "rdo_lambda", 0.0) > 0 or getattr(codec, "target_bytes", None) is not None
        imp_ = self.unembed(importance) if importance is not None and rdo_runs else (None, None)
        y_hat_ = side_params.new_zeros((2, n, c, h, w // 2))
        side_params_ = self.unembed(side_params)
        y_ = self.unembed(y)
        prepared = []
        body = self._head_parts()[0] if self.fuse_head else None
        for i in range(2):
            if self.fuse_head:  # (y, the features the head's last layer reads): the parameters are the encode kernel's business
                if codec.rdo_lambda > 0:
                    raise RuntimeError("rdo_lambda > 0 together with fuse_head is not supported")
                prepared.append((y_[i], body(self.merge(self._ctx(y_hat_, i), side_params_[i]))))
            else:
                params_i = self.entropy_parameters(self.merge(self._ctx(y_hat_, i), side_params_[i]))
                # (rdo_lambda = 0: the latent codec's own entry point, with its own setting - today's path)
                prepared.append(codec.coder_inputs_rdo(y_[i], params_i, self.rdo_lambda, imp_[i], self.rdo_channel_skip) if self.rdo_lambda > 0
                                else codec.coder_inputs(y_[i], params_i, imp_[i]) if imp_[i] is not None else codec.coder_inputs(y_[i], params_i))
            y_hat_[i] = torch.round(prepared[i][0])  # what compress() of this half returns as y_hat
        return prepared, self.embed(y_hat_)

    def finish(self, outs: List[Dict[str, Any]], y_hat: Tensor) -> Dict[str, Any]:
        """the two halves' coding results (``codec.compress_many``) -> the codec's result"""
        return {"strings": [o["strings"][0] for o in outs], "shape": y_hat.shape[1:], "y_hat": y_hat}

    def compress(self, y: Tensor, side_params: Tensor, importance: Optional[Tensor] = None) -> Dict[str, Any]:
        prepared, y_hat = self.prepare(y, side_params, importance)
        if self.fuse_head:
            return self.finish(self.latent_codec["y"].compress_many_head(prepared, self._head_parts()[1]), y_hat)
        return self.finish(self.latent_codec["y"].compress_many(prepared), y_hat)

    def estimate(self, y: Tensor, side_params: Tensor, **kwargs: Any) -> Dict[str, Any]:
        """The size of ``compress(y, side_params)``'s two bitstreams without coding them: ``prepare`` (the networks run as for
        ``compress``), then one size-estimate call for both halves.  -> ``{"estimates": [anchors, non-anchors] (RateEstimate),
        "bits_q", "bits", "nbytes"}``, the last three summed over the halves.  With ``fuse_head`` the parameters are the head's
        (``ParameterHead.params``, logits) - the ones its fused encode kernel codes with."""
        prepared, _ = self.prepare(y, side_params)
        codec = self.latent_codec["y"]
        if self.fuse_head:
            codec._check_head()
            ys, feats = zip(*prepared)
            scales, means, logits = self._head_parts()[1].params(torch.cat(list(feats)))
            est = codec.gaussian_mixture_conditional.estimate_bits_batch(torch.cat(list(ys)), scales, means, logits, weights_are_logits=True, **kwargs)
        else:
            est = codec.estimate_many(prepared, **kwargs)
        bits_q = sum(e.bits_q for e in est)
        return {"estimates": est, "bits_q": bits_q, "bits": bits_q / float(1 << 24), "nbytes": sum(e.nbytes for e in est)}

    def decompress(self, strings: List[Any], shape: Tuple[int, ...], side_params: Tensor, **kwargs: Any) -> Dict[str, Any]:
        n = 1
        c, h, w = shape
        codec = self.latent_codec["y"]
        y_hat_ = side_params.new_zeros((2, n, c, h, w // 2))
        y_rec_ = None  # the halves' "y_rec", where the latent codec gives one (its `centroid`); the context below keeps using y_hat
        side_params_ = self.unembed(side_params)
        for i in range(2):  # sequential by construction: the non-anchor parameters need the decoded anchors
            if self.fuse_head:
                body, head = self._head_parts()
                feat_i = body(self.merge(self._ctx(y_hat_, i), side_params_[i]))
                out = codec.decompress_many_head([[strings[i]]], (h, w // 2), [feat_i], head)[0]
            else:
                params_i = self.entropy_parameters(self.merge(self._ctx(y_hat_, i), side_params_[i]))
                out = codec.decompress([strings[i]], (h, w // 2), params_i)
            y_hat_[i] = out["y_hat"]
            if "y_rec" in out:
                y_rec_ = torch.zeros_like(y_hat_) if y_rec_ is None else y_rec_
                y_rec_[i] = out["y_rec"]
        if y_rec_ is None:
            return {"y_hat": self.embed(y_hat_)}
        return {"y_hat": self.embed(y_hat_), "y_rec": self.embed(y_rec_)}

    def decompress_many(self, strings: List[List[Any]], shape: Tuple[int, ...], side_params: List[Tensor]) -> List[Dict[str, Any]]:
        """N images of one shape, STAGE-MAJOR: the anchors of every image in one batched native call, then the non-anchors
        of every image in one — the dependency runs inside an image (checkerboard.py:316-324), not between images, so a
        call keeps N host decoders busy where ``decompress`` image by image keeps one."""
        c, h, w = shape
        codec = self.latent_codec["y"]
        y_hat_ = [sp.new_zeros((2, 1, c, h, w // 2)) for sp in side_params]
        y_rec_ = None  # (as in decompress)
        side_ = [self.unembed(sp) for sp in side_params]
        for i in range(2):
            if self.fuse_head:
                body, head = self._head_parts()
                feats = [body(self.merge(self._ctx(yh, i), sd[i])) for yh, sd in zip(y_hat_, side_)]
                outs = codec.decompress_many_head([[st[i]] for st in strings], (h, w // 2), feats, head)
            else:
                params = [self.entropy_parameters(self.merge(self._ctx(yh, i), sd[i])) for yh, sd in zip(y_hat_, side_)]
                outs = codec.decompress_many([[st[i]] for st in strings], (h, w // 2), params)
            for yh, o in zip(y_hat_, outs):
                yh[i] = o["y_hat"]
            if outs and "y_rec" in outs[0]:
                y_rec_ = [torch.zeros_like(yh) for yh in y_hat_] if y_rec_ is None else y_rec_
                for yr, o in zip(y_rec_, outs):
                    yr[i] = o["y_rec"]
        if y_rec_ is None:
            return [{"y_hat": self.embed(yh)} for yh in y_hat_]
        return [{"y_hat": self.embed(yh), "y_rec": self.embed(yr)} for yh, yr in zip(y_hat_, y_rec_)]

    def _check_mask(self) -> None:
        """forward()'s condition on context_prediction: a 5x5 convolution whose ``mask`` buffer is the checkerboard pattern.  Looked
        at once per mask (its address and version): the comparison reads the device back"""
        cp = self.context_prediction
        w, mask = getattr(cp, "weight", None), getattr(cp, "mask", None)
        if w is None or mask is None or w.dim() != 4 or tuple(w.shape[2:]) != (5, 5) or tuple(mask.shape) != tuple(w.shape):
            raise ValueError("forward() needs context_prediction to be a 5x5 convolution with a `mask` buffer of its weight's shape "
                             "(the reference's CheckerboardMaskedConv2d)")
        key = (mask.data_ptr(), mask._version, tuple(mask.shape))
        if getattr(self, "_mask_ok", None) == key:
            return
        keep = torch.zeros(25, dtype=torch.bool, device=mask.device)
        keep[1::2] = True  # the kernel positions (i, j) with i + j odd
        flat = mask.detach().reshape(mask.shape[0], mask.shape[1], 25)
        if not bool(((flat == 1) == keep).all()) or not bool(((flat == 0) == ~keep).all()):
            raise ValueError("context_prediction.mask is not the checkerboard pattern (1 at the kernel positions (i, j) with i + j odd, 0 elsewhere)")
        self._mask_ok = key

    def forward(self, y: Tensor, side_params: Tensor) -> Dict[str, Any]:
        """The reference's one-pass training forward (``_forward_onepass``, checkerboard.py:154-171; the only forward method the GMM
        models use, models/ckbd_gmm.py:125), any batch size: ``y_hat = y + U(-0.5, 0.5)`` in training, ``round(y)`` otherwise
        (:414-417); ``y_ctx`` = the context convolution of ``y_hat`` kept at the non-anchors, zeros at the anchors;
        ``params = entropy_parameters(merge(y_ctx, side_params))``; ``latent_codec["y"](y, params)`` ->
        ``{"likelihoods": {"y": ...}, "y_hat": y_hat}`` with this codec's own ``y_hat``, as the reference returns.

        ``fuse_context=False``: ``context_prediction`` runs as the torch module it is.  ``fuse_context=True``: a checkerboard-masked
        filter at a non-anchor reads only anchors, so ``y_ctx = embed([0, checkerboard_context(unembed(y_hat)[0], weight * mask,
        bias)])`` - the library's operator under autograd (header sections 5b, 5c: one fixed summation order forward and backward), the
        module's own ``forward`` never runs.  Its bits differ from MIOpen's: a model meant to be coded with ``fuse_context`` sees it in
        training.  ``context_prediction`` must carry a ``mask`` buffer equal to the checkerboard pattern (``ValueError`` otherwise).  A
        documented difference from the reference: the gradient of ``context_prediction.weight`` is that of ``weight * mask`` - +0 at
        the 13 dropped taps - where the reference, zeroing ``weight.data`` in place and differentiating a plain convolution
        (compressai/layers/layers.py:141-144), leaves non-zero values there that enter a global gradient-norm clip.

        ``fuse_head``, ``rdo_lambda`` / ``rdo_channel_skip`` and the inner codec's ``param_dtype`` are choices of the coding path and
        do not apply here.  The two-pass forward methods are not provided (the reference does not support them for GMM either)."""
        if self.forward_method != "onepass":
            raise NotImplementedError(f"forward_method {self.forward_method!r}: only \"onepass\" is provided, the one forward method the GMM models "
                                      "use (compressai/models/ckbd_gmm.py:125)")
        self._check_mask()
        if self.training:
            y_hat = y + torch.empty_like(y).uniform_(-0.5, 0.5)
        else:
            y_hat = torch.round(y)
        if self.fuse_context:
            cp = self.context_prediction
            ctx1 = checkerboard_context(self.unembed(y_hat)[0], cp.weight * cp.mask, getattr(cp, "bias", None), self.anchor_parity)
            y_ctx = self.embed(torch.stack([torch.zeros_like(ctx1), ctx1]))
        else:
            y_ctx = self.context_prediction(y_hat)
            keep = torch.zeros((1, 1) + tuple(y_ctx.shape[2:]), dtype=torch.bool, device=y_ctx.device)
            s = int(self.anchor_parity == "odd")  # non-anchors: (even row, odd column) and (odd row, even column) for "even"
            keep[..., 0::2, 1 - s::2] = True
            keep[..., 1::2, s::2] = True
            y_ctx = torch.where(keep, y_ctx, torch.zeros_like(y_ctx))  # _keep_only(., "non_anchor")
        params = self.entropy_parameters(self.merge(y_ctx, side_params))
        y_out = self.latent_codec["y"](y, params)
        return {"likelihoods": {"y": y_out["likelihoods"]["y"]}, "y_hat": y_hat}


class ChannelGroupsLatentCodec(nn.Module):
    """Channel groups coded one after the other, each conditioned on the previous ones (channel_groups.py:111-158);
    ``latent_codec[f"y{k}"]`` is typically a ``CheckerboardLatentCodec`` (models/elic_gmm.py:198-219)."""

    def __init__(self, latent_codec: Optional[Dict[str, nn.Module]] = None,
                 channel_context: Optional[Dict[str, nn.Module]] = None, *, groups: List[int], **kwargs: Any):
        super().__init__()
        self.groups = list(groups)
        self.groups_acc = list(accumulate(self.groups, initial=0))
        self.channel_context = nn.ModuleDict(channel_context)
        self.latent_codec = nn.ModuleDict(latent_codec)

    def __getitem__(self, key: str) -> nn.Module:
        return self.latent_codec[key]

    def merge_y(self, *args: Tensor) -> Tensor:
        return torch.cat(args, dim=1)

    def merge_params(self, *args: Tensor) -> Tensor:
        return torch.cat(args, dim=1)

    def _get_ctx_params(self, k: int, side_params: Tensor, y_hat_: Tuple[Tensor, ...]) -> Tensor:
        """parameters group k is coded under: the side parameters, preceded (k > 0) by the channel context computed
        from the reconstructions of groups 0..k-1 (channel_groups.py:166-173)"""
        if k == 0:
            return side_params
        return self.merge_params(self.channel_context[f"y{k}"](self.merge_y(*y_hat_[:k])), side_params)

    def _run(self, y_hat: Tensor, side_params: Tensor, code_group):
        """Groups in order; ``code_group(k, params) -> result dict`` codes one group and its ``"y_hat"`` becomes visible
        to the later groups through views of the one full-size ``y_hat`` tensor."""
        views = y_hat.split(self.groups, dim=1)
        results = []
        for k in range(len(self.groups)):
            res = code_group(k, self._get_ctx_params(k, side_params, views))
            views[k].copy_(res["y_hat"])
            results.append(res)
        return results

    @staticmethod
    def _one_call(codecs) -> bool:
        """can all groups be coded in one batched call?  (group codecs that can prepare, one Phi approximation, one clamp
        setting and one parameter dtype: what a batch of the entropy model must share)"""
        if any(getattr(c, "fuse_head", False) for c in codecs):  # (every group has a head of its own: group by group)
            return False
        try:
            keys = {(c.latent_codec["y"].gaussian_mixture_conditional._mode(), c.latent_codec["y"].gaussian_mixture_conditional.clamp_scales,
                     c.latent_codec["y"].param_dtype, c.latent_codec["y"].fuse_softmax) for c in codecs if hasattr(c, "prepare") and hasattr(c, "finish")}
        except (AttributeError, KeyError, TypeError):
            return False
        return len(keys) == 1 and all(hasattr(c, "prepare") for c in codecs)

    def compress(self, y: Tensor, side_params: Tensor) -> Dict[str, Any]:
        parts = torch.split(y, self.groups, dim=1)
        y_hat = torch.zeros_like(y)
        codecs = [self.latent_codec[f"y{k}"] for k in range(len(self.groups))]
        if self._one_call(codecs):
            # Every group's context is round(.) of data the encoder holds (channel_groups.py:117-120 hands over y_hat of
            # the groups before; on the encoder that is known without coding them), so the groups are PREPARED in order
            # and all their bitstreams are coded in ONE batched native call: ten host coders side by side, not ten calls.
            views = y_hat.split(self.groups, dim=1)
            prepared, hats = [], []
            for k, c in enumerate(codecs):
                pk, hk = c.prepare(parts[k], self._get_ctx_params(k, side_params, views))
                views[k].copy_(hk)
                prepared.append(pk)
                hats.append(hk)
            outs = codecs[0].latent_codec["y"].compress_many([p for pk in prepared for p in pk])
            results, at = [], 0
            for c, pk, hk in zip(codecs, prepared, hats):
                results.append(c.finish(outs[at:at + len(pk)], hk))
                at += len(pk)
        else:
            results = self._run(y_hat, side_params, lambda k, params: self.latent_codec[f"y{k}"].compress(parts[k], params))
        per_group = {len(r["strings"]) for r in results}
        if len(per_group) != 1:
            raise RuntimeError("every group codec must emit the same number of strings (channel_groups.py:124)")
        return {"strings": [s for r in results for s in r["strings"]], "shape": [r["shape"] for r in results], "y_hat": y_hat}

    def compress_many(self, ys: List[Tensor], side_params: List[Tensor]) -> List[Dict[str, Any]]:
        """``compress`` of N images: every image is prepared in group order (the networks run per image, batch 1 as the
        reference's), then ALL bitstreams of all images — N x groups x 2 — are coded in ONE batched native call."""
        codecs = [self.latent_codec[f"y{k}"] for k in range(len(self.groups))]
        if not self._one_call(codecs):
            return [self.compress(y, sp) for y, sp in zip(ys, side_params)]
        flat, per_image = [], []
        for y, sp in zip(ys, side_params):
            parts = torch.split(y, self.groups, dim=1)
            y_hat = torch.zeros_like(y)
            views = y_hat.split(self.groups, dim=1)
            prepared, hats = [], []
            for k, c in enumerate(codecs):
                pk, hk = c.prepare(parts[k], self._get_ctx_params(k, sp, views))
                views[k].copy_(hk)
                prepared.append(pk)
                hats.append(hk)
                flat.extend(pk)
            per_image.append((prepared, hats, y_hat))
        outs = codecs[0].latent_codec["y"].compress_many(flat)
        results, at = [], 0
        for prepared, hats, y_hat in per_image:
            rs = []
            for c, pk, hk in zip(codecs, prepared, hats):
                rs.append(c.finish(outs[at:at + len(pk)], hk))
                at += len(pk)
            results.append({"strings": [s_ for r in rs for s_ in r["strings"]], "shape": [r["shape"] for r in rs], "y_hat": y_hat})
        return results

    def decompress_many(self, strings: List[List[Any]], shape: List[Tuple[int, ...]], side_params: List[Tensor]) -> List[Dict[str, Any]]:
        """N images of one shape in flight, STAGE-MAJOR: group by group (channel_groups.py:147-154 — sequential inside an
        image), each group's stage of every image in one batched native call (``CheckerboardLatentCodec.decompress_many``).
        One image alone is a chain of single-bitstream calls — one host decoder at work, fifteen idle; N images fill the
        workers.  Results equal ``decompress`` image by image."""
        per_group = len(strings[0]) // len(self.groups)
        channels = sum(s_[0] for s_ in shape)
        y_hats = [torch.zeros((1, channels, *shape[0][1:]), device=sp.device) for sp in side_params]
        views = [yh.split(self.groups, dim=1) for yh in y_hats]
        recs = []  # per group, per image: the group codec's "y_rec" or None
        for k in range(len(self.groups)):
            codec = self.latent_codec[f"y{k}"]
            params = [self._get_ctx_params(k, sp, v) for sp, v in zip(side_params, views)]
            sub = [st[per_group * k: per_group * (k + 1)] for st in strings]
            if hasattr(codec, "decompress_many"):
                outs = codec.decompress_many(sub, shape[k], params)
            else:
                outs = [codec.decompress(st, shape[k], pr) for st, pr in zip(sub, params)]
            for v, o in zip(views, outs):
                v[k].copy_(o["y_hat"])
            recs.append([o.get("y_rec") for o in outs])
        res = [{"y_hat": yh} for yh in y_hats]
        if recs and all(r is not None for rs in recs for r in rs):  # every group's codec gives a "y_rec": concatenated; the context above keeps using y_hat
            for i, r in enumerate(res):
                r["y_rec"] = self.merge_y(*(rs[i] for rs in recs))
        return res

    def decompress(self, strings: List[Any], shape: List[Tuple[int, ...]], side_params: Tensor, **kwargs: Any) -> Dict[str, Any]:
        per_group = len(strings) // len(self.groups)
        channels = sum(s[0] for s in shape)
        y_hat = torch.zeros((1, channels, *shape[0][1:]), device=side_params.device)  # batch 1, as the reference (:139)
        results = self._run(y_hat, side_params, lambda k, params: self.latent_codec[f"y{k}"].decompress(
            strings[per_group * k: per_group * (k + 1)], shape[k], params))
        if results and all("y_rec" in r for r in results):  # concatenated; the channel context (_run) keeps using y_hat
            return {"y_hat": y_hat, "y_rec": self.merge_y(*(r["y_rec"] for r in results))}
        return {"y_hat": y_hat}

    def forward(self, y: Tensor, side_params: Tensor) -> Dict[str, Any]:
        """As the reference's (channel_groups.py:89-109): group k's codec is called with its slice of ``y`` and the parameters
        ``_get_ctx_params`` builds from the side parameters and the ``y_hat`` of groups 0 .. k-1; likelihoods and ``y_hat`` are
        concatenated along the channels."""
        y_ = torch.split(y, self.groups, dim=1)
        y_hat_: List[Tensor] = []
        y_likelihoods_: List[Tensor] = []
        for k in range(len(self.groups)):
            params = self._get_ctx_params(k, side_params, tuple(y_hat_))
            y_out = self.latent_codec[f"y{k}"](y_[k], params)
            y_hat_.append(y_out["y_hat"])
            y_likelihoods_.append(y_out["likelihoods"]["y"])
        return {"likelihoods": {"y": torch.cat(y_likelihoods_, dim=1)}, "y_hat": torch.cat(y_hat_, dim=1)}


class HyperLatentCodec(nn.Module):
    """Hyper branch (compressai/latent_codecs/hyper.py:48-108): ``z = h_a(y)`` is table-coded, ``params = h_s(z_hat)``.
    ``entropy_bottleneck`` is anything with the reference's ``compress(z) -> [bytes]`` / ``decompress(strings, size)``
    contract: ``flashgmm_amd.EntropyBottleneck`` (the density model and the tables; ``forward`` needs it or the reference's class),
    ``flashgmm_amd.EntropyBottleneckCoder`` (built from the tables of a trained ``EntropyBottleneck``), or the reference's own class."""

    def __init__(self, entropy_bottleneck=None, h_a: Optional[nn.Module] = None, h_s: Optional[nn.Module] = None,
                 quantizer: str = "noise", **kwargs: Any):
        super().__init__()
        assert entropy_bottleneck is not None
        self.entropy_bottleneck = entropy_bottleneck
        self.h_a = h_a or nn.Identity()
        self.h_s = h_s or nn.Identity()
        self.quantizer = quantizer

    def compress(self, y: Tensor) -> Dict[str, Any]:  # hyper.py:94-100
        z = self.h_a(y)
        shape = z.size()[-2:]
        eb = self.entropy_bottleneck
        if isinstance(eb, EntropyBottleneck):  # this package's module: its coding half, on its table buffers
            eb = eb.coder()
        if isinstance(eb, EntropyBottleneckCoder):
            # the reference decodes the strings it has just written to get z_hat (hyper.py:97-98); the table coder is lossless on
            # the symbols, so that is round(z - medians) + medians: one elementwise op where z lives, bit for bit the same
            z_strings, z_hat = eb.compress(z, return_dequantized=True)
        else:  # any other entropy bottleneck with the reference's contract
            z_strings = eb.compress(z)
            z_hat = eb.decompress(z_strings, shape)
        return {"strings": [z_strings], "shape": shape, "params": self.h_s(z_hat)}

    def decompress(self, strings: List[List[bytes]], shape: Tuple[int, int], **kwargs: Any) -> Dict[str, Any]:  # hyper.py:102-108
        (z_strings,) = strings
        z_hat = self.entropy_bottleneck.decompress(z_strings, shape)
        return {"params": self.h_s(z_hat)}

    def forward(self, y: Tensor) -> Dict[str, Any]:  # hyper.py:87-94
        """-> ``{"likelihoods": {"z": ...}, "params": h_s(z_hat)}``; ``entropy_bottleneck`` is ``flashgmm_amd.EntropyBottleneck`` (its
        density on the GPU, include/flashgmm_amd.h section 3j) or anything callable as the reference's class"""
        z = self.h_a(y)
        z_hat, z_likelihoods = self.entropy_bottleneck(z)
        if self.quantizer == "ste":
            d = z - self.entropy_bottleneck._get_medians()
            z_hat = ((torch.round(d) - d).detach() + d) + self.entropy_bottleneck._get_medians()  # quantize_ste (compressai/ops/ops.py:66-80)
        return {"likelihoods": {"z": z_likelihoods}, "params": self.h_s(z_hat)}


class HyperpriorLatentCodec(nn.Module):
    """``latent_codec = {"y": ..., "hyper": HyperLatentCodec}`` (compressai/latent_codecs/hyperprior.py:46-139): the complete
    nested result of the GMM models, ``{"strings": [*y_strings, z_strings], "shape": {"y": ..., "hyper": ...}, "y_hat"}``
    (models/ckbd_gmm.py:109-123: ``y`` is a ``CheckerboardLatentCodec``; models/elic_gmm.py:197-227: a
    ``ChannelGroupsLatentCodec``)."""

    def __init__(self, latent_codec: Optional[Dict[str, nn.Module]] = None, **kwargs: Any):
        super().__init__()
        if latent_codec is None or "y" not in latent_codec or "hyper" not in latent_codec:
            raise ValueError('latent_codec must hold the "y" and the "hyper" codec')
        self.latent_codec = nn.ModuleDict(latent_codec)

    def __getitem__(self, key: str) -> nn.Module:
        return self.latent_codec[key]

    def compress(self, y: Tensor) -> Dict[str, Any]:  # hyperprior.py:120-128
        hyper_out = self.latent_codec["hyper"].compress(y)
        y_out = self.latent_codec["y"].compress(y, hyper_out["params"])
        [z_strings] = hyper_out["strings"]
        return {"strings": [*y_out["strings"], z_strings], "shape": {"y": y_out["shape"], "hyper": hyper_out["shape"]},
                "y_hat": y_out["y_hat"]}

    def decompress(self, strings: List[Any], shape: Dict[str, Any], **kwargs: Any) -> Dict[str, Any]:  # hyperprior.py:130-139
        *y_strings_, z_strings = strings
        hyper_out = self.latent_codec["hyper"].decompress([z_strings], shape["hyper"])
        y_out = self.latent_codec["y"].decompress(y_strings_, shape["y"], hyper_out["params"])
        return {"y_hat": y_out["y_hat"]}

    def forward(self, y: Tensor) -> Dict[str, Any]:
        """As the reference's (hyperprior.py:109-118): the hyper codec's ``forward`` gives the ``z`` likelihoods and the parameters the
        ``y`` codec's ``forward`` runs under -> ``{"likelihoods": {"y": ..., "z": ...}, "y_hat": ...}``."""
        hyper_out = self.latent_codec["hyper"](y)
        y_out = self.latent_codec["y"](y, hyper_out["params"])
        return {"likelihoods": {"y": y_out["likelihoods"]["y"], "z": hyper_out["likelihoods"]["z"]}, "y_hat": y_out["y_hat"]}
