"""The arithmetic of include/flashgmm_amd.h section 3h - section 3g from the parameter head's logits - restated in torch, and the logits
corpus the tests of that section share.  Everything of section 3g itself is tests/like_ref.py's (``R``), unchanged.

``dlogits`` is the three lines of section 3h, one multiply or add per torch operation, so on float32 tensors it is the kernel's
arithmetic.  The float64 yardstick for the logits' gradient is ``reference_gradients_logits``: autograd through ``torch.softmax`` and
then through ``R.autograd_forward``.  ``mag`` is the magnitude of the terms a logit's gradient is a difference of,
pi_k * (|dpi_k| + sum_j pi_j |dpi_j|): dl_k = pi_k * (dpi_k - t) cancels where pi -> 1, and an error is measured against what cancels.

The logits corpus is ``R.corpus()``'s y, scales, means and g with the weights planes replaced by float32 logits, 2 * N(0, 1) from a
generator seeded with ``R.SEED + 7``, then per region of ``R.REGIONS``:

    (b)  one component at the row's maximum - 41.5 (softmax4 gives it exactly 0), another at the maximum - 40.5 (just inside)
    (d)  all four logits equal
    (e)  the largest raised by 20 to 30: pi ~ 1, the cancelling case of dpi_k - t
    (f)  a common offset of +80 or -80 on all four
    (a), (c), (g)  as drawn
"""
import numpy as np
import torch

from tests import like_ref as R

LOGIT_KINDS = ("nan", "pinf", "ninf", "all_ninf")


def _planes(rows):
    """[2048, 4] rows -> the [1, 32, 16, 16] layout of R.corpus()"""
    return np.ascontiguousarray(rows.reshape(8, 256, 4).transpose(2, 0, 1)).reshape(1, 32, 16, 16)


def logit_rows(planes):
    """[1, 32, 16, 16] planes -> [2048, 4] rows (a copy)"""
    return np.ascontiguousarray(np.asarray(planes).reshape(4, -1).T)


def logits_corpus(seed=R.SEED, sb=R.SB):
    """-> y, scales, means, logits, g as float32 arrays in R.corpus()'s layout"""
    y, sg, mu, _, g = R.corpus(seed, sb)
    rng = np.random.default_rng(seed + 7)
    lg = (2.0 * rng.standard_normal((2048, 4))).astype(np.float32)
    lo, hi = R.REGIONS["b"]
    top, at = lg[lo:hi].max(1), lg[lo:hi].argmax(1)
    rows = np.arange(lo, hi)
    lg[rows, (at + 1) % 4] = top - np.float32(41.5)
    lg[rows, (at + 2) % 4] = top - np.float32(40.5)
    lo, hi = R.REGIONS["d"]
    lg[lo:hi] = lg[lo:hi, :1]
    lo, hi = R.REGIONS["e"]
    rows = np.arange(lo, hi)
    at = lg[lo:hi].argmax(1)
    lg[rows, at] = (lg[rows, at] + rng.uniform(20.0, 30.0, hi - lo)).astype(np.float32)
    lo, hi = R.REGIONS["f"]
    lg[lo:hi] = (lg[lo:hi] + (80.0 * rng.choice([-1.0, 1.0], hi - lo))[:, None]).astype(np.float32)
    return y, sg, mu, _planes(lg), g


def nonfinite_logits(seed=R.SEED):
    """-> (y, scales, means, logits, g, planted): the logits corpus with a NaN logit, a +inf, a -inf and a row of four -inf planted,
    four of each, at distinct latents of region (a); ``planted`` lists (kind, flat latent index, component)"""
    y, sg, mu, lg, g = logits_corpus(seed)
    rows = logit_rows(lg)
    rng = np.random.default_rng(seed + 8)
    lo, hi = R.REGIONS["a"]
    at = lo + rng.choice(hi - lo, 4 * len(LOGIT_KINDS), replace=False)
    planted = []
    for j, i in enumerate(at.tolist()):
        kind, k = LOGIT_KINDS[j % len(LOGIT_KINDS)], int(rng.integers(0, 4))
        planted.append((kind, i, k))
        if kind == "all_ninf":
            rows[i] = -np.inf
        else:
            rows[i, k] = {"nan": np.nan, "pinf": np.inf, "ninf": -np.inf}[kind]
    return y, sg, mu, _planes(rows), g, planted


def softmax_planes(logits, dtype=torch.float64):
    """torch.softmax over K of [B, 4M, h, w] logits, in ``dtype`` -> planes of the same shape"""
    return torch.softmax(R._k(logits.to(dtype)), dim=1).reshape(logits.shape)


def dlogits(pi, dweights):
    """section 3h on planes [B, 4M, h, w]: t = ((pi_0*dpi_0 + pi_1*dpi_1) + pi_2*dpi_2) + pi_3*dpi_3, dl_k = pi_k * (dpi_k - t), each
    line one torch operation per IEEE operation (no addcmul: nothing is contracted)"""
    p, d = R._k(pi), R._k(dweights)
    t = p[:, 0] * d[:, 0]
    for k in range(1, 4):
        t = t + p[:, k] * d[:, k]
    dl = p * (d - t.unsqueeze(1))
    return dl.reshape(pi.shape)


def mag(pi, dweights):
    """float64: pi_k * (|dpi_k| + sum_j pi_j * |dpi_j|), the magnitude of the terms dl_k is a difference of -> planes"""
    p, d = R._k(pi.to(torch.float64)), torch.abs(R._k(dweights.to(torch.float64)))
    return (p * (d + (p * d).sum(1, keepdim=True))).reshape(pi.shape)


def reference_gradients_logits(y, scales, means, logits, g, rnd=False, sb=R.SB, lb=R.LB, dtype=torch.float64):
    """The float64 yardstick: autograd through torch.softmax on the [B, 4, M, h, w] view of the logits and then through
    R.autograd_forward -> (likelihood, dict of dy, dscales, dmeans, dweights - the last the gradient of the LOGITS)"""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (y, scales, means, logits)]
    weights = torch.softmax(R._k(leaves[3]), dim=1).reshape(leaves[3].shape)
    like = R.autograd_forward(torch.round(leaves[0]) if rnd else leaves[0], leaves[1], leaves[2], weights, sb, lb)
    like.backward(g.to(dtype))
    return like.detach(), dict(zip(R.GRADS, (t.grad for t in leaves)))
