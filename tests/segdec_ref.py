"""Shared by tests/test_segdec_ref_cpu.py and tests/test_gpu_segdec_edges.py: the STRUCTURAL edges of the GPU segment decoder
(segdec_kernel, flashgmm_amd/csrc/fgmm_tab.hip; its host side fgmm_decode_gpu.cpp), numpy only.

Two things live here.  A plain restatement of what the producer wave decides before any edge is evaluated - a latent's evaluation
window (``window_of``), the batches a segment falls into under the 2048-edge LDS budget (``plan_batches``), where the two producers
split a batch (``seam``) and which search a latent gets (``classify``) - and corpus builders whose items put chosen window lengths,
batch sizes, segment residues and bypass positions where the kernel changes its path.  Every parameter is ordinary (finite, sigma
positive and inside the clamp, positive weights that sum to 1, monotone rows), so the kernel must settle every item itself:
``ctx_stat(0, 4) == 1``.  tests/test_segdec_ref_cpu.py checks with these restatements and the oracle's own tables that each corpus
has the property it exists for.

A window's length depends on the saturation abscissae of the CDF approximation, so the builders that aim at a length take the
``mode``; items are ``(y [1, M, h, w], scales, means, weights [1, 4M, h, w])`` float32 like ``tests.synth.make_latent``."""
from __future__ import annotations

import functools

import numpy as np

from tests import edge_corpus as E
from tests import synth as T

F32 = np.float32
MODES = ("polya", "as", "logistic")
CAP_E = 2048         # fgmm_tab.hip kSegCapE: edges of one batch in LDS
PLAIN_MAX = 63       # fgmm_tab.hip slow_l: `len_l > 63u`
FREE_BS = 4000       # a half-width at which no window of these corpora is clipped by the table's ends


# ---- the planner, restated ------------------------------------------------------------------------------------------------------
def window_of(mode, mu, sg, pi, max_bs, clamp=True):
    """fgmm_decframe.h tab_window with prune = 1 in float32 numpy: rows ``mu, sg, pi [n, 4]`` -> ``(j_lo, j_hi)`` int64 [n], the indices
    (v = j - max_bs) between the saturated tails.  sigma goes through ``edge_corpus.clamp_sigma`` first when ``clamp``.

    The kernel computes ``tl`` and ``tr`` with one fmaf each, numpy with a rounded product and a rounded sum: where the two differ
    across a half-integer the window is off by one against the kernel's.  The corpora below sweep or repeat their lengths densely
    enough (and aim at the middle of a length's sigma range) that this does not matter; nothing here is compared with the kernel's
    window edge for edge."""
    mu, sg, pi = (np.asarray(a, F32).reshape(-1, 4) for a in (mu, sg, pi))
    if clamp:
        sg = E.clamp_sigma(sg)
    zl, zr = (F32(z) for z in E.SAT_Z[mode])
    W = 2 * int(max_bs) + 2
    w_ok = ((pi >= 0) & (pi <= 1)) if mode == "logistic" else np.isfinite(pi)
    ok = ((sg > 0) & np.isfinite(sg) & np.isfinite(mu) & w_ok).all(1)
    tl = (mu + (-zl) * sg).min(1)
    tr = (mu + zr * sg).max(1)
    lim = F32(max_bs) + F32(4)
    vl = np.clip(np.floor(tl + F32(0.5)) - F32(1), -lim, lim)
    vr = np.clip(np.ceil(tr + F32(0.5)) + F32(1), -lim, lim)
    ok_l = (((vl - F32(0.5))[:, None] - mu) / sg <= -zl).all(1)
    ok_r = (((vr - F32(0.5))[:, None] - mu) / sg >= zr).all(1)
    lo, hi = vl.astype(np.int64) + max_bs + 1, vr.astype(np.int64) + max_bs
    j_lo = np.where(ok & ok_l, np.clip(lo, 0, W), 0)
    j_hi = np.where(ok & ok_r, np.minimum(np.maximum(hi, j_lo), W), W)
    return j_lo, j_hi


def plan_batches(lengths, lo, hi):
    """producer step A for the segment [lo, hi): from ``base = lo`` a batch takes up to ``min(64, hi - base)`` latents, as many of them
    as keep ``2 * cumsum((len + 1) >> 1) <= 2048``, at least one -> [(base, nk, pairs)]"""
    lengths = np.asarray(lengths, np.int64)
    out, base = [], int(lo)
    while base < hi:
        nk_max = min(64, hi - base)
        incl = np.cumsum((lengths[base:base + nk_max] + 1) >> 1)
        nk = max(1, int((2 * incl <= CAP_E).sum()))
        out.append((base, nk, int(incl[nk - 1])))
        base += nk
    return out


def seam(NP):
    """the first pair of a batch's NP that the second producer evaluates"""
    return min(NP, ((NP * 7) // 16 + 63) & ~63)


def classify(length, j_lo, W):
    """"plain" (one pass of the wave) or "slow", by the clauses of slow_l that depend on shape alone: more than 63 edges, or a window
    that starts at index 0 - slow only when its first edge is not zero, which a window that the left tail did not cut usually is"""
    assert 0 <= j_lo and j_lo + length <= W, (length, j_lo, W)
    return "slow" if length > PLAIN_MAX or (j_lo == 0 and length > 0) else "plain"


def segments(n, stride):
    """[(lo, hi)] of the segments of an n-symbol stream"""
    return [(lo, min(lo + stride, n)) for lo in range(0, n, stride)]


# ---- items ----------------------------------------------------------------------------------------------------------------------
def planes(rows, M, h, w):
    """rows [M*h*w, 4] (channel-major latents) -> plane [1, 4M, h, w], component k at channel k*M + c"""
    return np.ascontiguousarray(np.asarray(rows, F32).reshape(M, h, w, 4).transpose(3, 0, 1, 2).reshape(1, 4 * M, h, w))


def item(y, sg, mu, pi, M, h, w):
    return np.ascontiguousarray(np.asarray(y, F32).reshape(1, M, h, w)), planes(sg, M, h, w), planes(mu, M, h, w), planes(pi, M, h, w)


def coded(it, clamp=True):
    """-> (symbols, sigma, mu, pi [n, 4] contiguous, abs_max, zero_bitmap): what the coder sees of an item, in coding order"""
    sym, s, m, w, am, zb, _ = T.to_coder_inputs(*(np.asarray(a, F32) for a in it), clamp=clamp)
    return sym, np.ascontiguousarray(s, F32), np.ascontiguousarray(m, F32), np.ascontiguousarray(w, F32), am, zb


def item_windows(mode, it, clamp=True):
    """-> (j_lo, j_hi, W) of an item's coded latents at the item's own half-width abs_max + 1"""
    _, s, m, w, am, _ = coded(it, clamp)
    j_lo, j_hi = window_of(mode, m, s, w, am + 1, clamp=clamp)
    return j_lo, j_hi, 2 * (am + 1) + 2


def _weights(rng, n):
    p = rng.uniform(0.2, 1.0, (n, 4))
    return (p / p.sum(1, keepdims=True)).astype(F32)


RATIOS = np.array([1.0, 0.9, 0.8, 0.7], F32)   # sigma_k / sigma_0 of a "smooth" latent
FRACS = np.array([0.1, 0.35, 0.6, 0.85], F32)   # mu_k - centre: the four means within one unit of each other


SHIFTS = (0.0, 0.37)  # a common shift of the four means: where both ends of a window move at the same sigma a length is skipped


@functools.lru_cache(maxsize=None)
def _sigma_table(mode):
    """window length -> (sigma_0, shift) of a smooth latent (sigma = sigma_0 * RATIOS, means = integer + shift + FRACS) that has it:
    the middle of the sigma range that gives the length, so that a last-bit difference in tl / tr does not move the window"""
    cand = np.geomspace(0.13, 255.0, 60000).astype(F32)
    out = {}
    for shift in SHIFTS:
        mu = np.tile(FRACS + F32(shift), (len(cand), 1))
        j_lo, j_hi = window_of(mode, mu, cand[:, None] * RATIOS, np.full((len(cand), 4), 0.25, F32), FREE_BS)
        ln = j_hi - j_lo
        for L in np.unique(ln):
            at = np.nonzero(ln == L)[0]
            out.setdefault(int(L), (float(cand[at[len(at) // 2]]), shift))
    return out


def sigma_for(mode, length):
    return _sigma_table(mode)[int(length)]


def _smooth(rng, mode, lengths, spread=3):
    """one smooth latent per requested window length -> (centre int [n], sigma, mu, pi [n, 4])"""
    n = len(lengths)
    s0, shift = (np.array(a, F32) for a in zip(*(sigma_for(mode, L) for L in lengths)))
    c = rng.integers(-spread, spread, n, endpoint=True)
    return c, s0[:, None] * RATIOS, ((c.astype(F32) + shift)[:, None] + FRACS).astype(F32), _weights(rng, n)


def _draw(rng, c, sg, lim):
    """symbols around the centre, well inside the window"""
    v = c + np.rint(rng.standard_normal(len(c)) * sg[:, 0] * 0.8)
    return np.clip(v, -lim, lim).astype(F32)


def ladder(seed, lo_len, hi_len, per, mode="polya"):
    """window lengths lo_len .. hi_len in turn, ``per`` consecutive latents each (sigma grows geometrically with the length, the four
    means within one unit).  PROPERTY: every length of the range occurs ``per`` times, so a boundary inside it - 63 | 64, plain | slow;
    64 | 65, 128 | 129: one, two, three passes of the slow search - has latents on both sides, next to each other in one batch."""
    rng = np.random.default_rng([seed, lo_len, hi_len])
    lengths = np.repeat(np.arange(lo_len, hi_len + 1), per)
    hw = 64
    M = -(-len(lengths) // hw)
    lengths = np.concatenate([lengths, np.full(M * hw - len(lengths), hi_len)])
    c, sg, mu, pi = _smooth(rng, mode, lengths)
    y = _draw(rng, c, sg, 200)
    y[3], y[-3] = F32(hi_len // 2 + 12), F32(-(hi_len // 2) - 12)  # a table wide enough for every window (two escapes)
    return item(y, sg, mu, pi, M, 8, 8)


BUDGET_LENGTHS = tuple(range(28, 41))
BUDGET_HW = 256


def budget(seed, mode="polya"):
    """one channel of 256 latents (= one segment at stride 256) per window length L = 28 .. 40: ``64 * ((L + 1) >> 1)`` crosses 1024
    from below - L = 31, 32 fill the 2048 edges exactly with 64 latents, L = 33 gives nk = 60; then a channel of L = 682 (nk = 3) and
    L = 700 (nk = 2), and one of L = 2040 at abs_max = 1022: one latent per batch, 32 passes of the slow search.
    PROPERTY: batches that the budget fills to the last edge, batches it cuts short, batches of one; seams inside a latent and on a
    latent's first pair."""
    rng = np.random.default_rng([seed, 7])
    lengths = np.concatenate([np.repeat(BUDGET_LENGTHS, BUDGET_HW), np.repeat([682, 700], BUDGET_HW // 2), np.full(BUDGET_HW, 2040)])
    M = len(lengths) // BUDGET_HW
    c, sg, mu, pi = _smooth(rng, mode, lengths, spread=1)
    wide = lengths == 2040
    lo_w, hi_w = window_of(mode, mu[wide][:1] - c[wide][:1, None].astype(F32), sg[wide][:1], pi[wide][:1], FREE_BS)
    c[wide] = -int(round((int(lo_w[0]) + int(hi_w[0])) / 2)) + FREE_BS  # the window's middle at v = 0: ZL != ZR puts it off the mean
    mu[wide] = (c[wide][:, None].astype(F32) + F32(sigma_for(mode, 2040)[1]) + FRACS).astype(F32)
    y = _draw(rng, c, sg, 1000)
    y[-1], y[-2] = F32(1021.25), F32(-1021.4)  # abs_max = 1022: the last half-width that is the kernel's
    return item(y, sg, mu, pi, M, 16, 16)


def full_width(seed, abs_max=40):
    """sigma 30 .. 60 at abs_max about 40: neither tail is saturated inside the table, the window is the whole row (j_lo = 0,
    j_hi = W) and its first edge is far from zero.  PROPERTY: `jl_l == 0 && first_l != 0`, the slow search with J counted from 0."""
    rng = np.random.default_rng([seed, 11])
    M, h, w = 3, 16, 16
    n = M * h * w
    sg = rng.uniform(30, 60, (n, 4)).astype(F32)
    mu = (rng.integers(-3, 3, n, endpoint=True)[:, None] + FRACS).astype(F32)
    y = np.clip(np.rint(rng.standard_normal(n) * 25), -(abs_max - 1), abs_max - 1).astype(F32)
    y[5], y[n - 7] = F32(abs_max - 1 + 0.6), F32(-(abs_max - 1) - 0.6)  # symbols +-abs_max; trunc(|y|) + 1 = abs_max
    return item(y, sg, mu, _weights(rng, n), M, h, w)


EXTREME_POS = ("j_lo-1", "j_lo", "j_lo+1", "j_hi-2", "j_hi-1", "j_hi")
EXTREME_LEN = (26.0, 60.0, 86.0)  # the wide components' reach: windows of about 30 (plain), 64 (the boundary: both) and 90 (slow) edges


def extreme_group(n):
    """index into EXTREME_LEN of the n latents of extremes(): runs of 18 (six positions x smooth | spike left | spike right)"""
    return (np.arange(n) // 18) % 3


def extremes(seed, mode="polya"):
    """plain (L about 30), slow (L about 90) and boundary (L = 60 .. 68) latents whose symbol sits at index j_lo - 1 .. j_lo + 1 or
    j_hi - 2 .. j_hi of their own window, EXTREME_POS in turn (latent i has position i % 6): the zeros below the window, its first and last intervals, the one that
    ends at the saturated tail, the first one inside the tail.  A third of the latents are smooth (such a symbol has frequency zero:
    bypass), a third carry a component of sigma 0.11 at the window's left end and a third at its right end, so that the CDF still
    moves in the window's outermost intervals (a regular symbol there).
    PROPERTY: the search's first and last lanes, `n - 1` and `n` at the ends of a window, both as a coded interval and as an escape."""
    rng = np.random.default_rng([seed, 13])
    zl, zr = E.SAT_Z[mode]
    M, h, w = 9, 8, 8
    n = M * h * w
    kind = (np.arange(n) // 6) % 3          # smooth | spike left | spike right
    s0 = np.array(EXTREME_LEN, np.float64)[extreme_group(n)] / (zl + zr) * rng.uniform(0.96, 1.04, n)
    c = rng.integers(-2, 2, n, endpoint=True)
    sg = (s0[:, None] * RATIOS).astype(F32)
    mu = (c[:, None] + FRACS).astype(F32)
    pi = _weights(rng, n)
    left, right = kind == 1, kind == 2
    sg[left | right, 3] = F32(0.11)
    # the narrow component lies half a unit beyond the wide ones' reach and so sets the window's end itself
    mu[left, 3] = (c[left] - zl * s0[left] - rng.uniform(0.3, 1.3, int(left.sum()))).astype(F32)
    mu[right, 3] = (c[right] + 0.8 + zr * s0[right] + rng.uniform(0.3, 1.3, int(right.sum()))).astype(F32)
    j_lo, j_hi = window_of(mode, mu, sg, pi, FREE_BS)
    pos = np.arange(n) % 6
    j = np.where(pos < 3, j_lo - 1 + pos, j_hi - 2 + (pos - 3))
    y = (j - FREE_BS).astype(F32)
    return item(y, sg, mu, pi, M, h, w)


def extreme_positions(mode, it):
    """-> (pos [n] index into EXTREME_POS, at [n] bool: the symbol sits where extremes() aimed it, at the item's own half-width)"""
    sym, *_, am, _ = coded(it)
    j_lo, j_hi, _ = item_windows(mode, it)
    pos = np.arange(len(sym)) % 6
    j = np.where(pos < 3, j_lo - 1 + pos, j_hi - 2 + (pos - 3))
    return pos, (sym.astype(np.int64) + am + 1) == j


BYPASS_VALUES = (7, -3, 0, 15, -1, 1, 0)  # one nibble; eight (a negative value: the int32 bit pattern); none at all
BYPASS_SHAPE = (8, 16, 16)                # 2048 latents: seven notes at stride 256


def bypass_positions(stride=256):
    """the default positions of bypass_at, in coding order"""
    n = int(np.prod(BYPASS_SHAPE))
    mid = 3 * stride
    return sorted({0,                                   # symbol 0 of the stream
                   stride - 1, stride,                  # last | first symbol of a segment: the note records the state after the nibbles
                   mid, mid + stride - 1,               # first and last symbol of a middle segment
                   mid + 63, mid + 64,                  # last | first latent of a 64-latent batch
                   n - 1,                               # the last symbol of the stream
                   *range(5 * stride + 30, 5 * stride + 100)})  # 70 escapes in a row: a whole batch of them and more


def bypass_at(seed, positions=None):
    """an ordinary latent (narrow windows: every batch holds 64 latents) with an outlier - a symbol 40 units below every mean, sigma 0.5:
    frequency zero in every mode - at each of ``positions`` (coding order; all channels are coded), the values BYPASS_VALUES in turn.
    PROPERTY: the escape's nibbles and refills at the first and last symbol of the stream, of a segment and of a batch, and a batch
    that consists of escapes; abs_max <= 16."""
    rng = np.random.default_rng([seed, 17])
    M, h, w = BYPASS_SHAPE
    n = M * h * w
    positions = bypass_positions() if positions is None else sorted(positions)
    sg = rng.uniform(0.5, 2.0, (n, 4)).astype(F32)
    mu = (rng.standard_normal((n, 1)) * 2 + rng.uniform(-0.5, 0.5, (n, 4))).astype(F32)
    y = np.rint(mu[:, 0] + rng.uniform(-0.4, 0.4, n) * sg[:, 0]).astype(F32)  # within half a sigma of a mean: never frequency zero
    for q, p in enumerate(positions):
        v = BYPASS_VALUES[q % len(BYPASS_VALUES)]
        y[p] = F32(v)
        sg[p] = F32(0.5)
        mu[p] = (v + 40 + FRACS).astype(F32)
    for ch in range(M):  # every channel stays coded, whatever the outliers did to it
        if not np.any(y[ch * h * w:(ch + 1) * h * w]):
            raise AssertionError("bypass_at: a channel without a symbol")
    return item(y, sg, mu, _weights(rng, n), M, h, w)


RESIDUES = (1, 2, 63, 64, 65, 255)
DEAD_PATTERNS = ("none", "first", "last", "alternating", "all_but_one", "first_200_of_300")


def dead_mask(pattern, M):
    """bool [M]: the channels without a coded symbol"""
    d = np.zeros(M, bool)
    if pattern == "first":
        d[0] = True
    elif pattern == "last":
        d[-1] = True
    elif pattern == "alternating":
        d[0::2] = True
    elif pattern == "all_but_one":
        d[:] = True
        d[M // 2] = False
    elif pattern == "first_200_of_300":
        assert M == 300
        d[:200] = True
    else:
        assert pattern == "none", pattern
    return d


def live_count(shape):
    M, h, w, pattern = shape
    return int((~dead_mask(pattern, M)).sum()) * h * w


def shapes(stride=256):
    """(M, h, w, dead-channel pattern): live counts n that take every residue against ``stride`` - n = stride * k + r for r in RESIDUES,
    n = stride * k exactly (k - 1 notes, a full last segment), n = stride + 1 (one symbol after the only note) - with every latent its
    own channel (h * w = 1), and at stride 256 channels of 7, 63, 65, 255 and 257 latents, where segment and batch boundaries fall in
    the middle of channels and one batch spans many, under every layout of dead channels.
    PROPERTY: `hi - base`, nk_max and `min(base + lane, hi - 1)` on short last segments; the live-then-dead channel list."""
    S = stride
    out = [(2 * S + r, 1, 1, "none") for r in RESIDUES] + [(2 * S, 1, 1, "none"), (S + 1, 1, 1, "none")]
    out += [(2 * (S + 63), 1, 1, "alternating")]                # n = S + 63, every other channel dead
    if S == 256:
        out += [(1, 1, 257, "none"),                  # n = 257 in one channel
                (3, 1, 257, "last"),                  # 514 = 2 * 256 + 2
                (6, 1, 257, "all_but_one"),           # 257, five dead channels around the live one
                (65, 7, 9, "none"),                   # 4095 = 15 * 256 + 255, channels of 63
                (65, 5, 13, "first"),                 # 64 live channels of 65: 4160 = 16 * 256 + 64
                (238, 1, 7, "alternating"),           # 119 live channels of 7: 833 = 3 * 256 + 65
                (300, 1, 7, "first_200_of_300"),      # 700 latents behind 200 dead channels
                (5, 15, 17, "none")]                  # channels of 255: 1275
    return out


def shape_item(seed, shape):
    """ordinary latents (tests.synth.make_latent) of that shape; dead channels quantise to all-zero, live ones hold a symbol"""
    M, h, w, pattern = shape
    y, sg, mu, pi = T.make_latent(seed, M=M, h=h, w=w)
    rng = np.random.default_rng([seed, 19])
    dead = dead_mask(pattern, M)
    y = y.copy()
    y[0, dead] = rng.uniform(-0.4, 0.4, (int(dead.sum()), h, w)).astype(F32)
    y = np.clip(y, -30, 30)
    flat = y[0].reshape(M, -1)
    quiet = ~dead & (np.rint(flat) == 0).all(1)
    flat[quiet, 0] = F32(1.0)  # (a view: y itself)
    return y, sg, mu, pi


def cheap_copy(it, upto):
    """the item with its first ``upto`` coded latents made very cheap (sigma 0.11 around the symbol itself: a frequency near 65535, a
    word of the stream every few hundred symbols): segments that rank last in the heaviest-first order.  All channels must be coded."""
    y, sg, mu, pi = (a.copy() for a in it)
    _, M, h, w = y.shape
    yq = np.rint(y).reshape(-1)
    for k in range(4):
        s_k, m_k = sg[0, k * M:(k + 1) * M].reshape(-1), mu[0, k * M:(k + 1) * M].reshape(-1)
        s_k[:upto] = F32(0.11)
        m_k[:upto] = yq[:upto]
    return y, sg, mu, pi
