"""The arithmetic of include/flashgmm_amd.h section 3k - the entropy bottleneck's update(): the quantile search, the integer support, the
masses of the support with the tail, the tables - restated in numpy and torch over tests/eb_ref.py, in float32 or float64, and the corpus
the update() tests share.

``bisect`` is the header's search, every (channel, target) on its own: a finished search is frozen, the others go on.  ``support`` is the
reference's float32 / int32 arithmetic (entropy_models.py:400-413).  ``masses`` evaluates ``eb_ref.forward`` (mode 0, no bound) on
``start + float32(i)`` - the samples are formed in float32 in either precision, as the kernel forms them - and the tail of :422, at the
channel's own last sample (the header's) or, ``tail_at_longest``, at the longest channel's as the reference takes it.  ``tables`` runs
``flashgmm_amd.ops.pmf_to_quantized_cdf`` on ``length + 1`` float32 entries per channel and pads with zeros (:206-214).

The corpus: the six channels of ``eb_ref.corpus()`` with quantiles bisected (float32) for tail_mass 1e-9, which gives the supports of
``LENGTHS``: none a multiple of a wave with its tail, the longest across several workgroups of the mass kernel; and a seventh channel, a copy of channel 1's
parameters whose three quantiles are equal: ``length`` 1, the smallest row.
"""
import numpy as np
import torch

from tests import eb_ref as R

TAIL_MASS = 1e-9
SEARCH_RADIUS = 1e5
LENGTHS = (321, 27, 212, 267, 139, 1022, 1)
C7 = len(LENGTHS)


def targets(tail_mass=TAIL_MASS):
    """the module's ``target`` buffer: float32 [3]"""
    t = float(np.log(2 / tail_mass - 1))
    return np.array([-t, 0.0, t], np.float32)


def as_tensors(params, dtype):
    return {n: torch.as_tensor(params[n]).to(dtype) for n in R.NAMES}


def bisect(params, dtype=torch.float32, tgt=None, radius=SEARCH_RADIUS, cap=256):
    """-> q [C, 3] (tensor of ``dtype``): the header's search; NaN where a chain value of the search was NaN.  ``cap``: steps at the most
    (the kernel's is 256, which binary32 never reaches on finite values; binary64 needs its own)"""
    P = as_tensors(params, dtype)
    Cn = P["_matrix0"].shape[0]
    t = torch.as_tensor(targets() if tgt is None else tgt).to(dtype).reshape(1, 3).expand(Cn, 3)
    f = lambda x: R.chain(P, x)  # noqa: E731
    lo, hi = torch.full((Cn, 3), -radius, dtype=dtype), torch.full((Cn, 3), radius, dtype=dtype)
    fv = f(hi)
    nan = torch.isnan(fv)
    lo = torch.where(t <= fv, lo, hi)
    fv = f(lo)
    nan = nan | torch.isnan(fv)
    hi = torch.where(fv <= t, hi, lo)
    done = nan.clone()
    for _ in range(cap):
        mid = (lo + hi) / 2
        done = done | (mid == lo) | (mid == hi)
        if bool(done.all()):
            break
        fv = f(mid)
        now = torch.isnan(fv) & ~done
        nan, done = nan | now, done | now
        lo, hi = torch.where(~done & (fv <= t), mid, lo), torch.where(~done & (fv >= t), mid, hi)
    q = (lo + hi) / 2
    q[nan] = float("nan")
    return q


def support(q):
    """q [C, 3] float32 (array) -> (offset int32 [C], start float32 [C], length int32 [C]): entropy_models.py:400-413"""
    q = np.asarray(q, np.float32)
    med = q[:, 1]
    minima = np.maximum(np.ceil(med - q[:, 0]).astype(np.int32), 0)
    maxima = np.maximum(np.ceil(q[:, 2] - med).astype(np.int32), 0)
    return -minima, (med - minima.astype(np.float32)).astype(np.float32), (maxima + minima + 1).astype(np.int32)


def samples(start, length):
    """-> float32 [C, max(length)]: start + float32(i), as torch adds arange(max_length) to pmf_start and as the kernel forms them"""
    return (np.asarray(start, np.float32)[:, None] + np.arange(int(np.max(length)), dtype=np.float32)[None, :]).astype(np.float32)


def masses(params, start, length, dtype=torch.float32, mirrored=True, tail_at_longest=False, device="cpu"):
    """-> (pmf [C, max(length)] with zeros from ``length`` on, tail [C]), arrays of ``dtype``"""
    length = np.asarray(length)
    s = torch.from_numpy(samples(start, length)).to(device)
    P = {n: t.to(device) for n, t in as_tensors(params, torch.float32).items()}
    f = R.forward(s[None], P, torch.zeros(len(length), device=device), 0, lb=0.0, dtype=dtype, mirrored=mirrored)
    L, lo, up = f["L"][0], f["lo"][0], f["up"][0]
    sig = lambda a: 1 / (1 + torch.exp(-a))  # noqa: E731
    last = torch.full((len(length), 1), s.shape[1] - 1, device=device) if tail_at_longest else torch.as_tensor(length - 1, device=device).long().reshape(-1, 1)
    tail = sig(lo[:, 0]) + sig(-up.gather(1, last)[:, 0])
    keep = torch.arange(s.shape[1], device=device)[None, :] < torch.as_tensor(length, device=device)[:, None]
    return torch.where(keep, L, torch.zeros_like(L)).cpu().numpy(), tail.cpu().numpy()


def tables(pmf, tail, length):
    """-> int32 [C, max(length) + 2]: per channel the quantised cumulative counts of its ``length`` masses and the tail, then zeros"""
    from flashgmm_amd import ops

    length = np.asarray(length)
    cdf = np.zeros((len(length), int(length.max()) + 2), np.int32)
    for c, n in enumerate(length.tolist()):
        prob = np.concatenate([pmf[c, :n], tail[c:c + 1]]).astype(np.float32)
        cdf[c, :n + 2] = ops.pmf_to_quantized_cdf(prob, 16)
    return cdf


def update(params, q, dtype=torch.float32, **kw):
    """the whole of update() on the quantiles q [C, 3] -> dict of offset, start, length, pmf, tail, cdf, cdf_length"""
    offset, start, length = support(q)
    pmf, tail = masses(params, start, length, dtype, **kw)
    return dict(offset=offset, start=start, length=length, pmf=pmf, tail=tail, cdf=tables(pmf, tail, length), cdf_length=length + 2)


FLOOR = 2.0 ** -17  # a mass below it rounds to a count of zero either way


def e_rel(x, x64, floor=FLOOR):
    """max |x - x64| / max(|x64|, floor): the project's error figure"""
    x64 = np.asarray(x64, np.float64)
    return float((np.abs(np.asarray(x, np.float64) - x64) / np.maximum(np.abs(x64), floor)).max())


def entries(pmf, tail, length, c):
    """channel c's ``length + 1`` entries as the quantiser gets them: its masses, then the tail"""
    n = int(np.asarray(length)[c])
    return np.concatenate([np.asarray(pmf)[c, :n], np.asarray(tail)[c:c + 1]])


def counts_of(prob32):
    """the quantiser's first step on float32 masses: round(p * 2^16) in float32, halves away from zero"""
    m = np.asarray(prob32, np.float32) * np.float32(65536.0)
    return np.floor(m.astype(np.float64) + 0.5).astype(np.int64)


def undecided(prob64, tau):
    """indices of the entries whose float64 mass m * 2^16 lies within tau * max(m * 2^16, 1) of a half-integer: round(m * 2^16), the
    quantiser's first step - the only place the masses enter the table - may go either way there; every other entry is DECIDED"""
    m = np.asarray(prob64, np.float64) * 65536.0
    return np.nonzero(np.abs(m - np.floor(m) - 0.5) <= tau * np.maximum(m, 1.0))[0].tolist()


def counts_admissible(prob32, prob64, tau):
    """the decided-entry rule on the masses a table was quantised from: float32 masses whose counts equal round(m64 * 2^16) at every
    decided entry and floor(m64 * 2^16) or that plus one at every undecided one -> (ok, undecided indices, indices that went the other way).
    A table IS the quantiser's function of these counts, so a table quantised from admissible counts is one of the tables obtained by
    rounding each undecided entry either way, however many there are."""
    m = np.asarray(prob64, np.float64) * 65536.0
    want, got, idx = np.floor(m + 0.5).astype(np.int64), counts_of(prob32), undecided(prob64, tau)
    off = np.nonzero(got != want)[0].tolist()
    ok = all(i in idx and got[i] in (np.floor(m[i]), np.floor(m[i]) + 1) for i in off)
    return ok, idx, off


def table_of_counts(counts):
    from flashgmm_amd import ops

    return np.asarray(ops.pmf_to_quantized_cdf((np.asarray(counts, np.float64) / 65536.0).astype(np.float32), 16), np.int32)


def table_admissible(row, prob64, tau, max_flips=2):
    """the decided-entry rule on a table alone (no masses to look at): ``row`` (length + 2 counts) equals the table of round(m64 * 2^16)
    with at most ``max_flips`` of the undecided entries rounded the other way -> (ok, undecided indices, the flipped ones or None).
    (Every subset would be admissible; two at the most keeps the search small and asks more.)"""
    import itertools

    m = np.asarray(prob64, np.float64) * 65536.0
    base, idx = np.floor(m + 0.5), undecided(prob64, tau)
    row = np.asarray(row[:len(m) + 1], np.int32)
    for k in range(max_flips + 1):
        for flip in itertools.combinations(idx, k):
            counts = base.copy()
            for i in flip:
                counts[i] = 2 * np.floor(m[i]) + 1 - counts[i]  # floor <-> floor + 1
            if np.array_equal(table_of_counts(counts), row):
                return True, idx, list(flip)
    return False, idx, None


_CORPUS = {}


def corpus():
    """-> dict: params {name: float32 array [7, ...]}, q32 / q64 [7, 3] (the bisected quantiles; channel 6: three equal ones),
    theta [7, 58] float32 (tensor); computed once, shared, not to be changed"""
    if not _CORPUS:
        _, p, _, _, _ = R.corpus()
        p7 = {n: np.concatenate([p[n], p[n][1:2]], 0) for n in R.NAMES}
        q32, q64 = bisect(p, torch.float32).numpy(), bisect(p, torch.float64, cap=4096).numpy()
        flat = np.float32(q32[1, 1])
        _CORPUS.update(params=p7, params6=p, q32=np.concatenate([q32, np.full((1, 3), flat, np.float32)], 0),
                       q64=np.concatenate([q64, np.full((1, 3), float(flat))], 0), theta=R.theta_of(p7).contiguous())
    return _CORPUS
