"""Shared by tests/test_sweep_ref_cpu.py and tests/test_gpu_symbol_sweep.py: the SYMBOL SWEEP corpus and its census, numpy only (the
search that refines the ladder asks the CPU oracle for row lengths; nothing of the product is imported).

A decoded symbol v consults exactly two entries of its row, F[v] and F[v + 1], and rANS advances its state with them: one wrong
visited entry desynchronises the rest of the stream.  A *sweep item* decodes every parameter set at every symbol of [-A, A], so
decoding it pins F_i[v] for v in [-A, A + 1] of every row in whichever table configuration decoded it - the tails, the entries
around the raw | Elias-Fano and 12-bit | 8-bit switches, the last entry before the trailing run, plateaus - and on the encode side
it drives the symbol-table, rate and fused encode kernels through every symbol of a row, zero-width intervals (bypass escapes)
included.

``ladder`` builds the monotone parameter sets, ``nonmono_sets`` the ones with a negative weight (kept in an item of their own: a
non-monotone row desynchronises the reference itself), ``sweep_item`` / ``sweep_item_by_channel`` lay them out, ``planes`` rounds
them to a 2-byte type, and ``census`` says from the oracle's full table what rows, blocks and shared words a configuration
(tl, ef_min) has.  tests/test_sweep_ref_cpu.py asserts with the oracle alone that the corpus has every property it exists for.

Items are ``(y [1, M, h, w], sigma, mu, pi [1, 4M, h, w])`` float32 like ``tests.synth.make_latent``, component k at channel k*M + c.
The symbols +-A are written as +-(A - 0.4): ``abs_max = trunc(max |y|) + 1`` is then A itself, the decoder's half-width A + 1."""
from __future__ import annotations

import functools

import numpy as np

from tests import bf16_planes as B
from tests import helpers
from tests import synth as T

F32 = np.float32
MODES = ("polya", "as", "logistic")
HALF_WIDTHS = (125, 126)     # abs_max: max_bs 126 (W = 254, the last 2-byte-header width) and 127 (W = 256, 4-byte headers)
P_SETS = 128
SHORT_LENGTHS = (13, 14, 15, 32, 33, 34, 48, 49, 50)  # around ef_min 14, 33, 49 and the 12-bit | 8-bit switch (48 | 49)
EF_MINS = (14, 33, 49)
CAP_DEFAULT, CAP_MAX, TL_MAX = 12288, 32768, 256      # fgmm_internal.h kTabCapE, the option's upper limit, kTabMaxTl
KINDS = ("sigma", "bimodal", "subunit", "f32only")


def width(A):
    """edges per row of the decoder's table at abs_max = A: v = -(A + 1) .. A + 2"""
    return 2 * (A + 1) + 2


def tab_tl(max_bs, cap_e):
    """fgmm_internal.h tab_tl restated: latents per block of the single-pass kernel at an LDS budget of cap_e edges (0: does not fit)"""
    t = (int(cap_e) // (2 * int(max_bs) + 2)) & ~15
    return min(t, TL_MAX) if t >= 16 else 0


def caps(A):
    """the three LDS budgets the GPU tests set: 16 rows, the default, the largest"""
    return (16 * width(A), CAP_DEFAULT, CAP_MAX)


# ---- parameter sets ---------------------------------------------------------------------------------------------------------------
def _sigma_sets(sig0, frac, scale=1.0):
    """one dominant component of sigma sig0 (weight 0.97) and three of sigma 0.3 (0.01 each), all four means at `frac`; weights * scale"""
    n = len(sig0)
    sg = np.full((n, 4), 0.3, F32)
    sg[:, 0] = sig0
    mu = np.repeat(np.asarray(frac, F32)[:, None], 4, 1)
    pi = np.tile((np.array([0.97, 0.01, 0.01, 0.01]) * scale).astype(F32), (n, 1))
    return sg, mu, pi


def _bimodal_sets(d, frac):
    """two tight pairs of components +-d apart (sigma 0.4, weight 1/4 each): the row is flat between them"""
    n = len(d)
    d, frac = np.asarray(d, np.float64), np.asarray(frac, np.float64)
    mu = np.stack([-d - 0.2, -d + 0.2, d - 0.2, d + 0.2], 1) + frac[:, None]
    return np.full((n, 4), 0.4, F32), mu.astype(F32), np.full((n, 4), 0.25, F32)


def f32_only_set():
    """a set none of whose values a 2-byte float holds (low mantissa bits set everywhere): the plane-type legs must round it"""
    sg = np.array([[1.2345678, 0.7654321, 2.3456789, 0.3141593]], F32)
    mu = np.array([[0.33333334, -1.2345678, 2.7182817, -0.5772157]], F32)
    pi = np.array([[0.4567891, 0.2345679, 0.1234567, 0.1851851]], F32)
    return sg, mu, pi


def trimmed_lengths(mode, sg, mu, pi, max_bs):
    """the oracle's rows -> cnt [n] of the trimmed rows (helpers._trim_row) at that half-width"""
    from oracle import oracle as O

    tab = O.cdftab(mode, sg, mu, pi, max_bs)
    return np.array([helpers._trim_row(r.astype(np.int64))[1] for r in tab])


def _first_with(lengths, want, taken):
    for i in np.nonzero(np.isin(lengths, want))[0]:
        if int(i) not in taken:
            return int(i)
    return None


@functools.lru_cache(maxsize=None)
def _ladder(mode, P):
    rng = np.random.default_rng([20, MODES.index(mode)])
    # the pools the search picks from: a dense sigma ladder and a dense bimodal family (d in quarter steps)
    n_s = 6000
    pool_s = _sigma_sets(np.geomspace(0.11, 256.0, n_s).astype(F32), rng.uniform(-0.95, 0.95, n_s))
    d_b = np.arange(3.0, 128.0, 0.25)
    pool_b = _bimodal_sets(d_b, rng.uniform(-0.45, 0.45, len(d_b)))
    len_s = {A: trimmed_lengths(mode, *pool_s, A + 1) for A in HALF_WIDTHS}
    len_b = {A: trimmed_lengths(mode, *pool_b, A + 1) for A in HALF_WIDTHS}
    same_s = len_s[125] == len_s[126]  # rows that neither table cuts: the same length at both half-widths
    same_b = len_b[125] == len_b[126]
    sets, kinds = [], []
    taken_s, taken_b = set(), set()

    def take(pool, i, kind):
        sets.append(tuple(a[i:i + 1] for a in pool))
        kinds.append(kind)

    def need(want, A=None):
        """one set whose trimmed length is in `want` - at both half-widths, or at A alone - from the sigma ladder, else a bimodal one"""
        ls = np.where(same_s, len_s[125], -1) if A is None else len_s[A]
        i = _first_with(ls, want, taken_s)
        if i is not None:
            taken_s.add(i)
            return take(pool_s, i, "sigma")
        lb = np.where(same_b, len_b[125], -1) if A is None else len_b[A]
        i = _first_with(lb, want, taken_b)
        assert i is not None, (mode, want, A)
        taken_b.add(i)
        take(pool_b, i, "bimodal")

    for L in SHORT_LENGTHS:
        need([L])
    need(list(range(64, 128)))
    need(list(range(128, width(125) - 1)))
    for A in HALF_WIDTHS:
        need([width(A) - 1], A)
        need([width(A)], A)
    # the families at large: bimodal d = 10 .. 85, sub-unit weights over the sigma range, the float32-only set, then the sigma ladder
    n_b, n_u = 12, 12
    take_b = _bimodal_sets(np.linspace(10.0, 85.0, n_b), rng.uniform(-0.45, 0.45, n_b))
    for i in range(n_b):
        take(take_b, i, "bimodal")
    take_u = _sigma_sets(np.geomspace(0.11, 256.0, n_u).astype(F32), rng.uniform(-0.95, 0.95, n_u), scale=0.8)
    for i in range(n_u):
        take(take_u, i, "subunit")
    take(f32_only_set(), 0, "f32only")
    rest = P - len(sets)
    assert rest >= 32, (P, len(sets))
    take_s = _sigma_sets(np.geomspace(0.11, 256.0, rest).astype(F32), rng.uniform(-0.95, 0.95, rest))
    for i in range(rest):
        take(take_s, i, "sigma")
    # A block of tl = 128 rows holds all P sets, so its bytes mod 4 are a property of the corpus: exchange a few of the last sigma rows
    # for pool rows until the sum is = 2 mod 4 under every (half-width, ef_min), the case in which tab_kernel pads the block.
    def parity(cnt125, cnt126):
        """[n] lengths at the two half-widths -> [n] bit vector over (A, ef_min) of (row bytes / 2) mod 2"""
        v = np.zeros(len(cnt125), np.int64)
        for a, cnt in enumerate((cnt125, cnt126)):
            ef = np.array([helpers.row_bytes(int(c), 0) for c in cnt])
            for e, ef_min in enumerate(EF_MINS):
                v |= ((np.where(cnt >= ef_min, ef, 2 * cnt) // 2) & 1) << (3 * a + e)
        return v

    cur = [np.concatenate([s[k] for s in sets]) for k in range(3)]
    v_rows = parity(*(trimmed_lengths(mode, *cur, A + 1) for A in HALF_WIDTHS))
    v_pool = parity(len_s[125], len_s[126])
    avail = {}
    for i in range(n_s):
        if i not in taken_s:
            avail.setdefault(int(v_pool[i]), []).append(i)
    state0 = int(np.bitwise_xor.reduce(v_rows))
    best = {state0: []}  # parity of the whole corpus -> [(row, pool vector)] that reaches it with the fewest exchanges
    for r in range(P - 1, P - 1 - 24, -1):
        for st, moves in list(best.items()):
            for u in avail:
                new = st ^ int(v_rows[r]) ^ u
                if sum(1 for _, uu in moves if uu == u) < len(avail[u]) and len(best.get(new, moves + [0, 0])) > len(moves) + 1:
                    best[new] = moves + [(r, u)]
    assert 63 in best, (mode, state0)
    for r, u in best[63]:
        i = avail[u].pop(len(avail[u]) // 2)
        sets[r] = tuple(a[i:i + 1] for a in pool_s)
    order = np.random.default_rng(7).permutation(P)  # neighbouring rows of a block differ in kind
    sg, mu, pi = (np.ascontiguousarray(np.concatenate([s[k] for s in sets])[order], F32) for k in range(3))
    return sg, mu, pi, tuple(kinds[i] for i in order)


def ladder(mode, P=P_SETS):
    """P monotone parameter sets -> (sigma, mu, pi) [P, 4] float32, every sigma in [0.11, 256] (the clamp is idle: one corpus serves
    clamp_scales True and False), shuffled with a fixed seed.  Refined by search against the oracle's table so that the trimmed row
    lengths SHORT_LENGTHS, one in [64, 128), one in [128, W - 2] and W - 1, W at both half-widths exist."""
    return _ladder(mode, P)[:3]


def ladder_kinds(mode, P=P_SETS):
    """the family of each set of ``ladder`` (KINDS), for failure messages and the census of families"""
    return _ladder(mode, P)[3]


def nonmono_sets(P=P_SETS):
    """sets with one negative weight, pi = (0.9, -0.3, 0.2, 0.2) over sigma = (1, 6, 0.4, 3) * s, s = 0.5 .. 3: the wide negative component
    makes the row fall in its flanks in every mode"""
    rng = np.random.default_rng(23)
    s = np.geomspace(0.5, 3.0, P)
    sg = (np.array([1.0, 6.0, 0.4, 3.0])[None, :] * s[:, None]).astype(F32)
    mu = np.repeat(rng.uniform(-0.95, 0.95, P)[:, None], 4, 1).astype(F32)
    pi = np.tile(np.array([0.9, -0.3, 0.2, 0.2], F32), (P, 1))
    return sg, mu, pi


# ---- items ------------------------------------------------------------------------------------------------------------------------
def _hw(n):
    h = max(d for d in range(1, int(n ** 0.5) + 1) if n % d == 0)
    return h, n // h


def _as_y(sym, A):
    """integer symbols -> the latent: +-A as +-(A - 0.4), so that trunc(max |y|) + 1 == A"""
    y = sym.astype(F32)
    y[sym == A] = F32(A - 0.4)
    y[sym == -A] = F32(-(A - 0.4))
    return y


def _planes(rows_cp, M, h, w):
    """[M, hw, 4] -> [1, 4M, h, w], component k at channel k*M + c"""
    return np.ascontiguousarray(np.asarray(rows_cp, F32).transpose(2, 0, 1).reshape(1, 4 * M, h, w))


def dead_channels(A, extra_dead=True):
    """the all-zero channels of sweep_item: one at the front, one in the middle"""
    return (0, A + 1) if extra_dead else ()


def sweep_item(sets, A, extra_dead=True):
    """S = 2A + 1 coded channels of hw = P positions, ``y[c, p] = ((c + p) mod S) - A``: position p carries parameter set p in every
    channel, so every set meets every symbol of [-A, A] exactly once as c runs, and no channel is constant.  With extra_dead an
    all-zero channel is inserted at the front and another in the middle: chan_list is not the identity."""
    sg, mu, pi = (np.asarray(a, F32) for a in sets)
    P, S = len(sg), 2 * A + 1
    h, w = _hw(P)
    sym = (np.arange(S)[:, None] + np.arange(P)[None, :]) % S - A
    dead = dead_channels(A, extra_dead)
    M = S + len(dead)
    live = np.array([c for c in range(M) if c not in dead])
    y = np.zeros((M, P), F32)
    y[live] = _as_y(sym, A)
    pl = [_planes(np.broadcast_to(a[None, :, :], (M, P, 4)), M, h, w) for a in (sg, mu, pi)]
    return (np.ascontiguousarray(y.reshape(1, M, h, w)), *pl)


def sweep_pairs(P, A):
    """coding order of sweep_item -> (set [n], symbol [n]) of every coded latent (dead channels are not coded)"""
    S = 2 * A + 1
    p = np.tile(np.arange(P), S)
    c = np.repeat(np.arange(S), P)
    return p, (c + p) % S - A


def sweep_item_by_channel(sets, A):
    """the transposed arrangement: channel c carries parameter set c at every position, the positions hold -A .. A and zeros up to
    h * w - whole blocks of identical rows"""
    sg, mu, pi = (np.asarray(a, F32) for a in sets)
    P, S = len(sg), 2 * A + 1
    h = w = int(np.ceil(np.sqrt(S)))
    sym = np.zeros((P, h * w), np.int64)
    sym[:, :S] = np.arange(-A, A + 1)[None, :]
    pl = [_planes(np.broadcast_to(a[:, None, :], (P, h * w, 4)), P, h, w) for a in (sg, mu, pi)]
    return (np.ascontiguousarray(_as_y(sym, A).reshape(1, P, h, w)), *pl)


def by_channel_pairs(P, A):
    """coding order of sweep_item_by_channel -> (set [n], symbol [n])"""
    S = 2 * A + 1
    hw = int(np.ceil(np.sqrt(S))) ** 2
    sym = np.zeros(hw, np.int64)
    sym[:S] = np.arange(-A, A + 1)
    return np.repeat(np.arange(P), hw), np.tile(sym, P)


def planes(a, kind):
    """the parameter planes (sigma, mu, pi) rounded to a 2-byte type -> (rounded planes, their float32 widening - what the oracle is fed).
    kind "f16": numpy float16 arrays (tests.synth.to_float16_planes); "bf16": uint16 bit patterns (tests.bf16_planes.planes_bits).
    sigma and mu round to nearest even; the weights round TOWARD ZERO in both helpers, so that their widened sum stays <= 1 and the
    rows stay monotone."""
    sg, mu, pi = a
    if kind == "f16":
        r = T.to_float16_planes(sg, mu, pi)
        return r, tuple(x.astype(F32) for x in r)
    assert kind == "bf16", kind
    r = B.planes_bits(sg, mu, pi, logits=False)
    return r, tuple(B.widen(x).reshape(x.shape) for x in r)


# ---- census -----------------------------------------------------------------------------------------------------------------------
def row_kind(cnt, nonmono, form, ef_min):
    if nonmono:
        return "escaped" if form == 2 else "raw"
    if ef_min is None or cnt < ef_min:
        return "raw"
    return "ef12" if helpers.ef_l(cnt) == 12 else "ef8"


def trim_rows(tab):
    """full table [n, W] -> int64 [n, 5]: a_idx, cnt, nonmono (helpers._trim_row), last entry, equal consecutive entries inside the
    trimmed row; each distinct row is trimmed once (a sweep item repeats its P rows)"""
    uniq, inv = np.unique(tab, axis=0, return_inverse=True)
    out = np.zeros((len(uniq), 5), np.int64)
    for i, F in enumerate(uniq.astype(np.int64)):
        a_idx, cnt, nm = helpers._trim_row(F)
        row = F[a_idx:a_idx + cnt]
        out[i] = a_idx, cnt, nm, row[-1], int((np.diff(row) == 0).sum())
    return out[inv.reshape(-1)]


def census(tab, max_bs, tl, ef_min, rows=None):
    """the oracle's full table [n, W] -> what the format of include/flashgmm_amd.h makes of it in blocks of ``tl`` rows with rows of at
    least ``ef_min`` entries Elias-Fano coded (None: no such rows); ``rows``: trim_rows(tab) where the caller has it already
      rows    int64 [n, 5]: a_idx, cnt, nonmono, last entry, equal consecutive entries inside the trimmed row
      kinds   [n] of "raw" | "ef12" | "ef8" | "escaped" (a non-monotone row behind a 2-byte header)
      bytes   int64 [n]: row bytes, an escaped row's 4-byte header included
      blocks  int64 [nblk]: the block's bytes mod 4 (2: the kernel pads it)
      shared  [(i, kind of row i + 1)]: adjacent rows of one block that share a 4-byte word - row i ends at offset % 4 == 2
      used    bytes of all blocks, each padded to 4"""
    n, W = tab.shape
    assert W == 2 * max_bs + 2
    form = helpers.hdr_form(max_bs)
    rows = trim_rows(tab) if rows is None else rows
    kinds, nbytes = np.empty(n, "<U7"), np.zeros(n, np.int64)
    for cnt, nm in np.unique(rows[:, 1:3], axis=0).tolist():
        k = row_kind(cnt, nm, form, ef_min)
        at = (rows[:, 1] == cnt) & (rows[:, 2] == nm)
        kinds[at] = k
        nbytes[at] = (helpers.row_bytes(cnt, nm) if k in ("ef12", "ef8") else 2 * cnt) + (4 if k == "escaped" else 0)
    blk = np.arange(n) // tl
    end = np.cumsum(nbytes)
    first = np.arange(0, n, tl)
    end = end - np.concatenate([[0], end])[first][blk]   # offset in its block at which row i ends
    last = np.minimum(first + tl, n) - 1
    at = np.nonzero((end % 4 == 2) & (np.arange(n) != last[blk]))[0]
    shared = [(int(i), str(kinds[i + 1])) for i in at]
    return {"rows": rows, "kinds": kinds, "bytes": nbytes, "blocks": end[last] % 4, "shared": shared, "used": int(((end[last] + 3) & ~3).sum())}
