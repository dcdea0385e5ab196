"""Shared by tests/test_enc_forms_cpu.py, tests/test_gpu_enc_forms.py and the GPU modules of the encode-frame family: which of its four
launch forms a call that prices latents takes - ``estimate_bits``, ``quantize_rdo``, ``rd_curve``, ``quantize_to_budget``, their weighted
forms (include/flashgmm_amd.h section 3e) and their channel-skip forms (3f) - and ``ODD_CORPUS``, the smallest planes at which each
form can go wrong.

``latent_launch_form`` restates the launcher's decision (flashgmm_amd/csrc/fgmm_estimate.cpp ``LatentFrame::start`` with
fgmm_encode.cpp ``enc_vec4_ok``): ONE form - 4 positions per lane or 1, the linear grid or the tiled one - for the whole batch.
``items_of`` reads the items off the tensors a call is really handed (``data_ptr``, shape, strides), so a test asserts the form of its
call, not the form it believes a shape has; ``planned_items`` gives the same items for a corpus entry without a device.

Every corpus entry is a latent of ``tests/synth.make_latent`` with its dead channels PLANTED (non-zero latents that all round to zero:
the compact channel list matters at every size), every live channel rescaled until something of it is coded, one live channel made
faint (something to skip) and, in two entries, one outlier far outside a narrow mixture (a bypass escape, and a channel that may never
be skipped).  numpy only."""
from __future__ import annotations

import numpy as np

from tests import bf16_planes as BF
from tests import rdo_weights_ref as W
from tests import synth as T

LIN, TILED = True, False
WAVE = 64
PLANE_TYPES = ("f32", "f16", "bf16")
MODES = ("polya", "as", "logistic")
LAM = 0.5  # the lambda of the non-vacuity conditions
LAMBDAS3 = (0.0, 0.5, 5.0)
LAMBDAS16 = (0.0, 0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 16.0)
FORMS4 = ((False, False), (True, False), (False, True), (True, True))  # (weighted, skip): plain, weighted, skip, weighted + skip


# ---- the launcher's decision ------------------------------------------------------------------------------------------------------------
def form_item(hw, stride_c, stride_k, planes, y, out=0):
    """one item as ``latent_launch_form`` reads it: ``planes`` the byte addresses of scales, means and weights, ``y`` that of the latent,
    ``out`` that of what the call's kernel writes per latent (y_rdo, the per-latent map), 0 where the call has none"""
    return dict(hw=int(hw), stride_c=int(stride_c), stride_k=int(stride_k), planes=tuple(int(p) for p in planes), y=int(y), out=int(out))


def latent_launch_form(items, two_byte, pos_w_ptrs=None):
    """``LatentFrame::start`` and ``enc_vec4_ok`` restated -> (vec, linear) of the ONE launch that serves every item.  4 per lane needs,
    of every item, hw, stride_c and stride_k multiples of 4, the three planes aligned to 4 elements (16 bytes, 8 for two-byte planes), y
    and the output to 16 bytes and - ``pos_w_ptrs``: the call is weighted - every pos_w pointer (0: the item has none) to 16 bytes.
    The grid is linear only if every hw is a multiple of 64 * vec."""
    plane_mask = 7 if two_byte else 15
    vec4 = True
    for i, it in enumerate(items):
        ok = all(x % 4 == 0 for x in (it["hw"], it["stride_c"], it["stride_k"])) and all(p & plane_mask == 0 for p in it["planes"])
        ok = ok and it["y"] % 16 == 0 and it["out"] % 16 == 0
        if pos_w_ptrs is not None:
            ok = ok and int(pos_w_ptrs[i]) % 16 == 0
        vec4 = vec4 and ok
    vec = 4 if vec4 else 1
    return vec, all(it["hw"] % (WAVE * vec) == 0 for it in items)


def _plane_item(s, m, w, y_ptr, out):
    """one item from its [1, 4M, h, w] planes, the address of its latent and that of its output (0: none)"""
    KM, h, wd = s.shape[1], s.shape[2], s.shape[3]
    hw = h * wd
    for t in (s, m, w):  # what ops take as they are: dense (h, w) planes, one channel stride for the three (anything else is copied)
        assert tuple(t.shape) == tuple(s.shape) and t.stride() == s.stride() and (hw <= 1 or (t.stride(3) == 1 and t.stride(2) == wd)), "not plane-dense"
    stride_c = s.stride(1) if KM > 1 else hw
    return form_item(hw, stride_c, (KM // 4) * stride_c, [t.data_ptr() for t in (s, m, w)], y_ptr, out)


def items_of(ys, scales, means, weights, outs=None):
    """the items of a call, from the device tensors handed over: sequences of [1, M, h, w] / [1, 4M, h, w] tensors, or stacked
    [N, ...] tensors (item i at batch offset i).  ``outs``: the per-latent outputs of the call, once it has returned them (they are
    fresh allocations; before the call the form is asserted with them taken as aligned, after it with their addresses)"""
    if hasattr(ys, "data_ptr"):  # stacked
        N = ys.shape[0]
        assert ys.is_contiguous()
        return [_plane_item(scales[i:i + 1], means[i:i + 1], weights[i:i + 1], ys.data_ptr() + 4 * i * ys.stride(0),
                            0 if outs is None else outs[i].data_ptr()) for i in range(N)]
    items = []
    for i, (y, s, m, w) in enumerate(zip(ys, scales, means, weights)):
        assert y.is_contiguous() and y.element_size() == 4
        items.append(_plane_item(s, m, w, y.data_ptr(), 0 if outs is None else outs[i].data_ptr()))
    return items


def form_of(ys, scales, means, weights, pos_w=None, outs=None):
    """-> (vec, linear) of the call on these tensors; ``pos_w``: the call's position weights, one tensor (or None) per item"""
    first = scales if hasattr(scales, "data_ptr") else scales[0]
    ptrs = None if pos_w is None else [0 if t is None else t.data_ptr() for t in pos_w]
    return latent_launch_form(items_of(ys, scales, means, weights, outs), first.element_size() == 2, ptrs)


def form_of_one(y, s, m, w, pos_w=None, out=None):
    """``form_of`` for a single call; ``pos_w``: False - the call is not weighted -, None - weighted without position factors -, or the tensor"""
    return form_of([y], [s], [m], [w], None if pos_w is False else [pos_w], None if out is None else [out])


# ---- the corpus -------------------------------------------------------------------------------------------------------------------------
# (M, h, w, placement).  placement: "dense" - every tensor an allocation of its own; "y_off" - y a dense view one float into its storage;
# "stride" - planes whose channel stride is hw + 2 (dense rows in a larger storage); "pos_w_off" - in the weighted calls, pos_w one
# float into its storage
ODD_CORPUS = [
    (1, 1, 1, "dense"),      # hw = 1                      1-wide, tiled: less than one 4-wide load, a wave with one active lane
    (3, 1, 3, "dense"),      # hw = 3
    (4, 3, 7, "dense"),      # hw = 21                     channel rows 4-byte aligned (2-byte with two-byte planes)
    (5, 7, 9, "dense"),      # hw = 63                     one lane short of a wave
    (2, 5, 13, "dense"),     # hw = 65                     one lane alone in a second wave
    (3, 15, 17, "dense"),    # hw = 255                    one lane short of a workgroup
    (2, 1, 257, "dense"),    # hw = 257                    one lane alone in a second workgroup
    (1, 2, 2, "dense"),      # hw = 4                      4-wide, tiled: one lane
    (4, 12, 21, "dense"),    # hw = 252                    63 lanes
    (5, 13, 20, "dense"),    # hw = 260                    65 lanes: one alone in a second wave
    (3, 8, 8, "y_off"),      # hw = 64                     1-wide, linear: one wave per channel
    (2, 8, 16, "y_off"),     # hw = 128                    two
    (4, 16, 16, "dense"),    # hw = 256                    4-wide, linear
    (3, 4, 4, "stride"),     # hw = 16, stride_c = 18      1-wide by stride alone
    (4, 4, 4, "pos_w_off"),  # hw = 16                     1-wide by pos_w alone (4-wide in the calls without weights)
]
# the planted dead channels of each entry: "first", "last", "all_but_one" (the survivor: channel M // 2), "none"; an entry with M = 1 has none
DEAD = ["none", "first", "last", "all_but_one", "none", "first", "last", "none", "none", "first", "last", "none", "all_but_one", "first", "last"]
OUTLIER = (5, 9)  # entries with one latent the coder bypasses, in their last live channel: 1-wide tiled and 4-wide tiled
SEED = 7100


def dead_channels(i):
    M, how = ODD_CORPUS[i][0], DEAD[i]
    return {"none": [], "first": [0], "last": [M - 1], "all_but_one": [c for c in range(M) if c != M // 2]}[how]


def corpus_case(i, clamp):
    """entry i -> (y, scales, means, weights) float32 in tests/synth.make_latent's layout; ``clamp``: the test clamps - sigma is then
    handed over un-clamped, as the sibling modules do"""
    M, h, w, _ = ODD_CORPUS[i]
    hw = h * w
    y, s, m, pi = T.make_latent(SEED + i, M, h, w, clamp=not clamp)
    y, s, m = y.copy(), s.copy(), m.copy()
    dead = dead_channels(i)
    live = [c for c in range(M) if c not in dead]
    rng = np.random.default_rng(SEED + 100 + i)
    for c in dead:  # latents that are not zero and all round to zero
        y[0, c] = rng.uniform(0.05, 0.49, (h, w)).astype(np.float32) * rng.choice([-1.0, 1.0], (h, w)).astype(np.float32)
    for c in live:  # something of every live channel is coded, and nothing of it lies beyond FGMM_SKIP_VMAX
        top = float(np.abs(y[0, c]).max())
        if top < 1.3 or top > 14.0:
            y[0, c] = (y[0, c] * np.float32(min(max(top, 1.3), 14.0) / top)).astype(np.float32)
    if len(live) >= 2:  # a faint channel: a few +-1 among zeros, under a mixture that makes them dear
        c = live[1]
        y[0, c] = (y[0, c] * np.float32(0.8 / float(np.abs(y[0, c]).max()))).astype(np.float32)
        for k in range(4):
            s[0, k * M + c], m[0, k * M + c] = np.float32(0.3), np.float32(0.0)
    if i in OUTLIER:  # v0 = 40 under sigma = 0.2 at 0: its range quantises to zero, the coder takes the bypass escape
        c, p = live[-1], hw // 2
        y[0, c].reshape(-1)[p] = np.float32(40.2)
        for k in range(4):
            s[0, k * M + c].reshape(-1)[p], m[0, k * M + c].reshape(-1)[p] = np.float32(0.2), np.float32(0.0)
    return y, s, m, pi


def planes_of(case, plane_type):
    """-> (what the device is handed: float32 / float16 arrays or bfloat16 bit patterns, the float32 values they stand for)"""
    s, m, pi = case[1:]
    if plane_type == "f32":
        return (s, m, pi), (s, m, pi)
    if plane_type == "f16":
        p = T.to_float16_planes(s, m, pi)
        return p, tuple(a.astype(np.float32) for a in p)
    p = (BF.bf16_rne(s), BF.bf16_rne(m), BF.bf16_trunc(pi))  # the weights toward zero: their sum stays <= 1
    return p, tuple(BF.widen(a).reshape(s.shape) for a in p)


def widened_case(i, clamp, plane_type):
    """entry i as the reference is fed it: y and the float32 values of the planes of ``plane_type``"""
    case = corpus_case(i, clamp)
    return (case[0],) + planes_of(case, plane_type)[1]


def factors(i):
    """entry i's fixed factors of section 3e -> (chan_w [M], pos_w [h, w])"""
    M, h, w, _ = ODD_CORPUS[i]
    return W.chan_w(M), W.pos_w(h * w).reshape(h, w)


def planned_items(i, weighted):
    """entry i as a call of its own, without a device -> (items, pos_w_ptrs or None): every allocation at address 0, the placement's
    offset added.  tests/test_gpu_enc_forms.py asserts that the tensors it builds give the same form"""
    M, h, w, placement = ODD_CORPUS[i]
    hw = h * w
    stride_c = hw + 2 if placement == "stride" else hw
    item = form_item(hw, stride_c, M * stride_c, (0, 0, 0), 4 if placement == "y_off" else 0)
    return [item], ([4 if placement == "pos_w_off" else 0] if weighted else None)


def planned_form(i, plane_type, weighted):
    items, pos_w_ptrs = planned_items(i, weighted)
    return latent_launch_form(items, plane_type != "f32", pos_w_ptrs)


def entries_of_form(form, plane_type="f32", weighted=False):
    """the corpus entries that run in ``form`` as calls of their own"""
    return [i for i in range(len(ODD_CORPUS)) if planned_form(i, plane_type, weighted) == form]


def instantiations():
    """what the cases tests/test_gpu_enc_forms.py derives from the corpus launch -> (rate, rdoq, rdcurve): sets of
    (mode, vec, clamped, plane type, linear) for rate_kernel and (..., weighted, skip) for the two others.  Every entry is run by
    every (mode, clamp, plane type), rate once and RDOQ and the curve in the four forms of FORMS4"""
    rate, rdoq = set(), set()
    for mode in MODES:
        for clamp in (True, False):
            for pt in PLANE_TYPES:
                for i in range(len(ODD_CORPUS)):
                    vec, linear = planned_form(i, pt, False)
                    rate.add((mode, vec, clamp, pt, linear))
                    for weighted, skip in FORMS4:
                        vec, linear = planned_form(i, pt, weighted)
                        rdoq.add((mode, vec, clamp, pt, linear, weighted, skip))
    return rate, rdoq, set(rdoq)
