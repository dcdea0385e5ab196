"""CPU: the structural corpus of the GPU segment decoder (tests/segdec_ref.py) does what it claims.  Every property is derived from
the restated planner (window_of, plan_batches, seam, classify) and the oracle's own tables (oracle.cdftab / oracle.symtab); nothing
comes from the library under test.  tests/test_gpu_segdec_edges.py then runs these items through segdec_kernel."""
import functools

import numpy as np
import pytest

from tests import segdec_ref as S

MODES = list(S.MODES)
STRIDE = 256


@functools.lru_cache(maxsize=None)
def corpus(mode):
    return {
        "ladder_63": S.ladder(1, 56, 72, 16, mode),
        "ladder_128": S.ladder(2, 120, 136, 16, mode),
        "budget": S.budget(3, mode),
        "full_width": S.full_width(4),
        "full_width_short": S.full_width(5, abs_max=25),
        "extremes": S.extremes(6, mode),
        "bypass_at": S.bypass_at(7),
    }


def _lengths(mode, it):
    j_lo, j_hi, W = S.item_windows(mode, it)
    return j_hi - j_lo, j_lo, W


def _batches(mode, it):
    """-> [(base, nk, pairs, nk_max)] of every segment of the item at stride 256, and the lengths"""
    ln, _, _ = _lengths(mode, it)
    out = []
    for lo, hi in S.segments(len(ln), STRIDE):
        out += [(b, nk, p, min(64, hi - b)) for b, nk, p in S.plan_batches(ln, lo, hi)]
    return out, ln


def test_planner_restatement_on_hand_made_rows():
    assert S.seam(1024) == 448 and S.seam(1020) == 448 and S.seam(10) == 10 and S.seam(0) == 0 and S.seam(146) == 64
    assert S.plan_batches(np.full(256, 32), 0, 256) == [(0, 64, 1024), (64, 64, 1024), (128, 64, 1024), (192, 64, 1024)]
    assert S.plan_batches(np.full(256, 33), 0, 256) == [(0, 60, 1020), (60, 60, 1020), (120, 60, 1020), (180, 60, 1020), (240, 16, 272)]
    assert S.plan_batches(np.full(300, 2046), 256, 259) == [(256, 1, 1023), (257, 1, 1023), (258, 1, 1023)]
    assert S.plan_batches(np.zeros(70, int), 0, 70) == [(0, 64, 0), (64, 6, 0)]
    assert S.classify(63, 5, 100) == "plain" and S.classify(64, 5, 100) == "slow" and S.classify(20, 0, 100) == "slow"
    # one component, sigma 1, mean 0, half-width 20: polya's tails saturate 5.25 below and 5.0 above the mean
    j_lo, j_hi = S.window_of("polya", [[0, 0, 0, 0]], [[1, 1, 1, 1]], [[0.25] * 4], 20)
    assert (int(j_lo[0]), int(j_hi[0])) == (-6 + 20 + 1, 7 + 20)
    j_lo, j_hi = S.window_of("polya", [[0, 0, 0, 0]], [[0.01] * 4], [[0.25] * 4], 20)  # clamped to 0.11
    assert (int(j_lo[0]), int(j_hi[0])) == (-2 + 20 + 1, 3 + 20)
    j_lo, j_hi = S.window_of("polya", [[0, 0, 0, 0]], [[50] * 4], [[0.25] * 4], 20)  # no tail inside the table
    assert (int(j_lo[0]), int(j_hi[0])) == (0, 42)


@pytest.mark.parametrize("mode", MODES)
def test_ladder_covers_both_sides_of_every_length_boundary(mode):
    for name, lo, hi in (("ladder_63", 58, 70), ("ladder_128", 122, 134)):
        ln, j_lo, W = _lengths(mode, corpus(mode)[name])
        count = np.bincount(ln, minlength=hi + 1)
        assert all(count[L] >= 4 for L in range(lo, hi + 1)), (name, count[lo:hi + 1])
        assert (np.diff(ln) >= 0).all() and len(ln) > STRIDE, name  # grows along the item (the padding repeats the last length)
    ln, j_lo, W = _lengths(mode, corpus(mode)["ladder_63"])
    kinds = {S.classify(int(L), int(j), W) for L, j in zip(ln, j_lo)}
    assert kinds == {"plain", "slow"}
    # the boundary itself sits inside one batch: a batch with latents of 63 and of 64 edges
    batches, ln = _batches(mode, corpus(mode)["ladder_63"])
    assert any({63, 64} <= set(ln[b:b + nk].tolist()) for b, nk, _, _ in batches)


@pytest.mark.parametrize("mode", MODES)
def test_budget_fills_cuts_and_splits_batches(mode):
    it = corpus(mode)["budget"]
    batches, ln = _batches(mode, it)
    assert S.coded(it)[4] == 1022
    for k, L in enumerate(S.BUDGET_LENGTHS):  # one length per segment
        assert (ln[k * 256:(k + 1) * 256] == L).all(), (L, np.unique(ln[k * 256:(k + 1) * 256]))
    assert any(nk == 64 and 1920 < 2 * p <= 2048 for _, nk, p, _ in batches)
    assert any(nk == 64 and 2 * p == 2048 for _, nk, p, _ in batches)
    assert any(nk < 64 and nk < nk_max for _, nk, _, nk_max in batches)  # cut by the budget, not by the segment's end
    assert any(nk == 60 for _, nk, _, _ in batches)
    assert {1, 2, 3} <= {nk for _, nk, _, nk_max in batches if nk < nk_max}
    assert (np.abs(ln[-256:] - 2040) <= 2).all() and all(nk == 1 for b, nk, _, _ in batches if b >= len(ln) - 256)  # 32 passes of 64 lanes
    inside = on_first = 0
    for b, nk, p, _ in batches:
        offs = np.concatenate([[0], np.cumsum((ln[b:b + nk] + 1) >> 1)])
        h = S.seam(p)
        if 0 < h < p:
            on_first += h in offs[1:-1].tolist()
            inside += h not in offs.tolist()
    assert inside > 0 and on_first > 0


@pytest.mark.parametrize("mode", MODES)
def test_full_width_is_the_whole_row_with_a_first_edge(oracle, mode):
    for name, am_want in (("full_width", 40), ("full_width_short", 25)):
        it = corpus(mode)[name]
        sym, s, m, w, am, _ = S.coded(it)
        ln, j_lo, W = _lengths(mode, it)
        assert am == am_want and (j_lo == 0).all() and (ln == W).all()
        tab = oracle.cdftab(mode, s, m, w, am + 1)
        assert (tab[:, 0] > 0).all()
        assert sym.min() == -am and sym.max() == am
    assert 2 * 26 + 2 <= S.PLAIN_MAX < 2 * 41 + 2  # slow by the first edge alone | by its length as well


# The positions a regular symbol can take.  tab_window leaves one index of slack at either end for the rounding of tl and tr: the edge
# at j_lo is still 0 and the edge at j_hi - 1 is already the saturated one.  The intervals j_lo - 1 = [0, F[j_lo]), j_hi - 1 =
# [F[j_hi - 1], T_sat) and j_hi = [T_sat, T_sat) are therefore EMPTY for ordinary parameters: a symbol there is always an escape.
REGULAR_POS = ("j_lo", "j_lo+1", "j_hi-2")
ALWAYS_BYPASS_POS = ("j_lo-1", "j_hi-1", "j_hi")


@pytest.mark.parametrize("mode", MODES)
def test_outermost_window_edges_are_saturated_even_where_the_rounding_is_tight(oracle, mode):
    """the slack above, hunted: rows whose narrow component (sigma 0.11 .. 0.33) puts tl + 0.5 or tr + 0.5 within a few float32 ulps of
    an integer - where the window's end is decided by one rounding - still have F[j_lo] == 0 and F[j_hi - 1] == T_sat.  This is why
    no VALID stream tells `len_l > 63u` from `len_l > 64u` in segdec_kernel: a 64-edge window searched in one pass goes wrong only
    when all 64 edges are <= cf or none is, and cf >= F[j_hi - 1] = T_sat or cf < F[j_lo] = 0 is no regular symbol's (tests/
    test_gpu_segdec_edges.py therefore pins that boundary by decoding both sides of it, not by telling the two searches apart)."""
    rng = np.random.default_rng(23)
    zl, zr = S.E.SAT_Z[mode]
    n, bs = 120000, 200
    s0 = rng.uniform(2, 7, n)
    sg = (s0[:, None] * S.RATIOS).astype(np.float32)
    sg[:, 3] = np.float32(0.11) * rng.choice([1, 1.5, 2, 3], n).astype(np.float32)
    mu = (rng.integers(-2, 3, n)[:, None] + S.FRACS).astype(np.float32)
    right = np.arange(n) % 2 == 0
    nudge = rng.choice([-2e-6, -1e-6, -5e-7, 0, 5e-7, 1e-6, 2e-6], n)
    at_right = np.rint(zr * s0 + 3) + 0.5 - np.float32(zr) * sg[:, 3]
    at_left = np.rint(-zl * s0 - 3) + 0.5 + np.float32(zl) * sg[:, 3]
    mu[:, 3] = np.where(right, at_right, at_left) + nudge
    pi = rng.uniform(0.2, 1, (n, 4))
    pi = (pi / pi.sum(1, keepdims=True)).astype(np.float32)
    j_lo, j_hi = S.window_of(mode, mu, sg, pi, bs)
    assert {63, 64, 65} <= set((j_hi - j_lo).tolist())

    def q16(c):
        return np.trunc(c.astype(np.float32) * np.float32(65535)).astype(np.int64)

    f_last, _ = oracle.gmm_cdf(mode, (j_hi - 1 - bs).astype(np.int32), sg, mu, pi)  # the lower edge of v: F[v + bs]
    f_first, _ = oracle.gmm_cdf(mode, (j_lo - bs).astype(np.int32), sg, mu, pi)
    assert (q16(f_last) == q16((pi[:, 0] + pi[:, 1]) + (pi[:, 2] + pi[:, 3]))).all() and (q16(f_first) == 0).all()


@pytest.mark.parametrize("mode", MODES)
def test_extremes_sit_at_the_ends_of_their_windows(oracle, mode):
    it = corpus(mode)["extremes"]
    sym, s, m, w, am, _ = S.coded(it)
    ln, j_lo, W = _lengths(mode, it)
    pos, at = S.extreme_positions(mode, it)
    assert at.all() and 2 * (am + 1) + 2 <= 2048
    rng_ = oracle.symtab(mode, sym, s, m, w) >> 16
    grp = S.extreme_group(len(sym))
    plain = ln <= S.PLAIN_MAX
    assert plain[grp == 0].all() and 20 <= ln[grp == 0].min() and ln[grp == 0].max() <= 45
    assert not plain[grp == 2].any() and 75 <= ln[grp == 2].min() and ln[grp == 2].max() <= 110
    assert {62, 63, 64, 65} <= set(ln[grp == 1].tolist()) and 55 <= ln[grp == 1].min() and ln[grp == 1].max() <= 75
    for q, name in enumerate(S.EXTREME_POS):
        cells = (("plain", grp == 0), ("slow", grp == 2), ("boundary, plain", (grp == 1) & plain), ("boundary, slow", (grp == 1) & ~plain))
        for which, sel in cells:
            here = sel & (pos == q)
            assert here.sum() >= 8, (name, which)
            assert (rng_[here] == 0).any(), (name, which, "no escape")
            if name in REGULAR_POS:
                assert (rng_[here] > 0).any(), (name, which, "no regular symbol")
            else:
                assert name in ALWAYS_BYPASS_POS and (rng_[here] == 0).all(), (name, which)


@pytest.mark.parametrize("mode", MODES)
def test_bypass_at_escapes_exactly_where_asked(oracle, mode):
    it = corpus(mode)["bypass_at"]
    sym, s, m, w, am, zb = S.coded(it)
    want = S.bypass_positions()
    assert zb.all() and am <= 1022 and am <= 16
    got = np.nonzero((oracle.symtab(mode, sym, s, m, w) >> 16) == 0)[0].tolist()
    assert got == want
    _, nb = oracle.encode_gmm(mode, sym, s, m, w, return_bypass=True)
    assert nb == len(want) and len(want) == 78
    n = len(sym)
    assert {0, 255, 256, n - 1} <= set(want) and {3 * 256 + 63, 3 * 256 + 64} <= set(want)
    assert {7, -3, 0, 15} <= set(sym[want].tolist())
    ln, _, _ = _lengths(mode, it)
    assert all(nk == 64 for _, nk, _ in S.plan_batches(ln, 768, 1024))  # 63 | 64 is a batch boundary


def test_shapes_take_every_residue():
    for stride in (256, 512, 2048):
        ns = [S.live_count(sh) for sh in S.shapes(stride)]
        assert all(n > stride for n in ns)  # at least one note: the item is the kernel's
        assert set(S.RESIDUES) | {0} <= {n % stride for n in ns}
        assert stride + 1 in ns and any(n % stride == 0 for n in ns)
    sh = S.shapes(256)
    assert {1, 7, 63, 65, 255, 257} <= {h * w for _, h, w, _ in sh} and 257 in [S.live_count(x) for x in sh]
    assert (513, 1, 1, "none") in sh and set(S.DEAD_PATTERNS) <= {p for *_, p in sh}
    for shape in sh:
        it = S.shape_item(20, shape)
        zb = S.coded(it)[5]
        assert (zb == 0).tolist() == S.dead_mask(shape[3], shape[0]).tolist(), shape


@pytest.mark.parametrize("mode", MODES)
def test_every_item_is_valid_monotone_and_round_trips(oracle, mode):
    items = dict(corpus(mode))
    items.update({f"shape{sh}": S.shape_item(20 + k, sh) for k, sh in enumerate(S.shapes(256))})
    items["cheap"] = S.cheap_copy(corpus(mode)["bypass_at"], 1024)
    for name, it in items.items():
        sym, s, m, w, am, _ = S.coded(it)
        assert np.isfinite(s).all() and (s >= 0.11).all() and (s <= 256).all() and np.isfinite(m).all(), name
        assert (w > 0).all() and np.abs(w.astype(np.float64).sum(1) - 1).max() < 1e-6, name
        assert 2 * (am + 1) + 2 <= 2048 and len(sym) > STRIDE, name
        tab = oracle.cdftab(mode, s, m, w, am + 1).astype(np.int32)
        assert (np.diff(tab, axis=1) >= 0).all(), name
        enc = oracle.encode_gmm(mode, sym, s, m, w)
        assert np.array_equal(oracle.decode_gmm(mode, enc, s, m, w, am + 1), sym), name
