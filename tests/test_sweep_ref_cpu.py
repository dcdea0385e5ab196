"""CPU: the symbol-sweep corpus of tests/sweep_ref.py has the properties tests/test_gpu_symbol_sweep.py relies on - by the oracle alone.
These are CONDITIONS, not measurements: without them the GPU tests could pass vacuously (a corpus without a row of 33 entries says
nothing about ef_min = 33).  If one fails, the corpus has to change until the reference alone meets it."""
import functools
import itertools

import numpy as np
import pytest

from tests import helpers
from tests import sweep_ref as W
from tests import synth as T

MODES = list(W.MODES)
# block sizes per half-width: tab_tl at 16 * W edges, at the default 12288 and at 32768.  At A = 126 (W = 256) the default gives
# 12288 / 256 = 48 rows; 32 is checked as well, a block size between the two that the option can also produce (cap_e = 8192)
TLS = {125: (16, 48, 128), 126: (16, 32, 48, 128)}


@functools.lru_cache(maxsize=None)
def tables(oracle, mode, A):
    """-> (ladder table [P, W], non-monotone table [P, W]) at the decoder's half-width A + 1"""
    return oracle.cdftab(mode, *W.ladder(mode), A + 1), oracle.cdftab(mode, *W.nonmono_sets(), A + 1)


@functools.lru_cache(maxsize=None)
def coded(oracle, mode, A, which):
    """-> (symbols, sigma, mu, pi, abs_max, bytes, bypass count, the oracle's decode) of an item"""
    sets = W.nonmono_sets() if which == "nonmono" else W.ladder(mode)
    it = W.sweep_item_by_channel(sets, A) if which == "by_channel" else W.sweep_item(sets, A)
    sym, s, m, w, am, zb, _ = T.to_coder_inputs(*it)
    b, nb = oracle.encode_gmm(mode, sym, s, m, w, return_bypass=True)
    return sym, s, m, w, am, b, nb, oracle.decode_gmm(mode, b, s, m, w, am + 1), zb


def test_tab_tl_restated():
    """fgmm_internal.h tab_tl in numpy: the block sizes of the three LDS budgets the GPU tests set"""
    for A in W.HALF_WIDTHS:
        assert W.width(A) == {125: 254, 126: 256}[A] and helpers.hdr_form(A + 1) == {125: 2, 126: 4}[A]
        assert [W.tab_tl(A + 1, c) for c in W.caps(A)] == [16, 48, 128]
    assert W.tab_tl(127, 8192) == 32 and W.tab_tl(127, 16 * 256 - 1) == 0 and W.tab_tl(5, 32768) == 256
    assert all(set(W.tab_tl(A + 1, c) for c in W.caps(A)) <= set(TLS[A]) for A in W.HALF_WIDTHS)


@pytest.mark.parametrize("mode", MODES)
def test_ladder_parameters(mode):
    sg, mu, pi = W.ladder(mode)
    kinds = W.ladder_kinds(mode)
    assert sg.shape == mu.shape == pi.shape == (W.P_SETS, 4) and sg.dtype == np.float32 and len(kinds) == W.P_SETS
    assert sg.min() >= np.float32(0.11) and sg.max() <= np.float32(256)  # the clamp is idle
    assert (pi > 0).all() and set(kinds) == set(W.KINDS)
    sub = np.array(kinds) == "subunit"
    assert sub.sum() >= 8 and np.allclose(pi[sub].sum(1), 0.8, atol=1e-6) and np.allclose(pi[~sub].sum(1), 1.0, atol=1e-6)
    f = np.array(kinds) == "f32only"
    assert f.sum() == 1
    for a in (sg[f], mu[f], pi[f]):  # no value of that set survives a 2-byte type
        assert (a.astype(np.float16).astype(np.float32) != a).all()
        assert (W.B.widen(W.B.bf16_rne(a)).reshape(a.shape) != a).all()
    # shuffled: the families are not sorted into runs
    assert max(len(list(g)) for k, g in itertools.groupby(kinds) if k != "sigma") <= 3
    assert len(W.ladder(mode, 121)[0]) == 121


@pytest.mark.parametrize("A", W.HALF_WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_row_lengths(oracle, mode, A):
    tab, _ = tables(oracle, mode, A)
    r = W.census(tab, A + 1, 48, 33)["rows"]
    Wd = W.width(A)
    assert not r[:, 2].any()  # monotone, every one
    have = set(r[:, 1].tolist())
    assert set(W.SHORT_LENGTHS) <= have, sorted(set(W.SHORT_LENGTHS) - have)
    assert any(64 <= L < 128 for L in have) and any(128 <= L <= Wd - 2 for L in have)
    assert {Wd - 1, Wd} <= have, sorted(have)[-4:]
    assert (r[:, 3] < 65535).sum() >= 8 and (r[:, 3] == 65535).sum() >= 8
    assert (r[:, 4] > 0).sum() >= 8  # a plateau: equal consecutive entries inside the row
    kinds = np.array(W.ladder_kinds(mode))
    assert (r[kinds == "bimodal", 4] > 0).all()
    # the sub-unit rows that saturate inside the table end at T_sat = quant16(0.8), far below 65535
    sub = r[kinds == "subunit"]
    assert (sub[:, 3] < 65535).all() and (sub[:, 0] + sub[:, 1] < Wd).sum() >= 6


@pytest.mark.parametrize("A", W.HALF_WIDTHS)
def test_symbol_coverage(A):
    P = W.P_SETS
    sets = W.ladder("polya")
    y, sg, mu, pi = W.sweep_item(sets, A)
    sym, s, m, w, am, zb, yq = T.to_coder_inputs(y, sg, mu, pi)
    S = 2 * A + 1
    assert am == A and y.shape[1] == S + 2 and zb.tolist() == [int(c not in W.dead_channels(A)) for c in range(S + 2)]
    p, v = W.sweep_pairs(P, A)
    assert np.array_equal(v, sym) and len(sym) == P * S
    assert np.array_equal(np.ascontiguousarray(s), sets[0][p]) and np.array_equal(np.ascontiguousarray(w), sets[2][p])
    seen = np.zeros((P, S), np.int64)
    np.add.at(seen, (p, v + A), 1)
    assert (seen == 1).all()  # every (set, symbol) pair exactly once
    live = np.rint(y[0, np.nonzero(zb)[0]].reshape(S, -1))
    assert (live.min(1) != live.max(1)).all()  # no channel is constant
    assert np.array_equal(W.sweep_item(sets, A, extra_dead=False)[0][0].reshape(S, -1), y[0, np.nonzero(zb)[0]].reshape(S, -1))
    # the transposed arrangement: every pair at least once, the padding is symbol 0 of the same set
    yc, sgc, muc, pic = W.sweep_item_by_channel(sets, A)
    symc, sc, _, _, amc, zbc, _ = T.to_coder_inputs(yc, sgc, muc, pic)
    pc, vc = W.by_channel_pairs(P, A)
    assert amc == A and zbc.all() and np.array_equal(vc, symc) and np.array_equal(np.ascontiguousarray(sc), sets[0][pc])
    seen = np.zeros((P, S), np.int64)
    np.add.at(seen, (pc, vc + A), 1)
    assert (seen >= 1).all() and (np.delete(seen, A, 1) == 1).all()


@pytest.mark.parametrize("which", ["sweep", "by_channel"])
@pytest.mark.parametrize("A", W.HALF_WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_oracle_decodes_the_monotone_items(oracle, mode, A, which):
    """so the GPU tests may demand both: the decode equals the oracle's, and it equals round(y)"""
    sym, s, m, w, am, b, nb, dec, _ = coded(oracle, mode, A, which)
    assert am == A and np.array_equal(dec, sym)
    assert 0.25 <= nb / len(sym) <= 0.75, nb / len(sym)  # bypass escapes and coded intervals, both well represented


@pytest.mark.parametrize("A", W.HALF_WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_block_structure(oracle, mode, A):
    """the table of the sweep item's coded latents (its P rows, repeated channel by channel) in every configuration the GPU tests
    decode it under: a block the kernel has to pad, and rows of every kind that start in the middle of a 4-byte word"""
    tab, _ = tables(oracle, mode, A)
    p, _ = W.sweep_pairs(W.P_SETS, A)
    trimmed = W.trim_rows(tab)
    for tl in TLS[A]:
        for ef_min in W.EF_MINS:
            for t, r in ((tab, trimmed), (tab[p], trimmed[p])):  # the P rows as test (g) builds them, and the item's own table
                c = W.census(t, A + 1, tl, ef_min, rows=r)
                assert (c["blocks"] == 2).any(), (tl, ef_min, len(t))
                second = {k for _, k in c["shared"]}
                want = {"raw", "ef8"} | ({"ef12"} if ef_min <= 48 else set())
                assert second == want, (tl, ef_min, second)
                assert c["used"] == int(c["bytes"].sum()) + 2 * int((c["blocks"] == 2).sum())
    # without Elias-Fano rows (ef_rows = 2, FGMM_TAB_RAW_ROWS) every row is raw
    c = W.census(tab, A + 1, 48, None)
    assert set(c["kinds"].tolist()) == {"raw"} and np.array_equal(c["bytes"], 2 * c["rows"][:, 1])


@pytest.mark.parametrize("A", W.HALF_WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_nonmonotone_item(oracle, mode, A):
    _, tab = tables(oracle, mode, A)
    c = W.census(tab, A + 1, 48, 14)
    r = c["rows"]
    assert r[:, 2].all()  # every row is non-monotone ...
    assert (r[:, 1] >= 14).any()  # ... long enough for Elias-Fano, and must stay raw
    assert set(c["kinds"].tolist()) == {"escaped" if A == 125 else "raw"}
    if A == 125:  # behind 2-byte headers such a row is escaped: its 4-byte header starts in the middle of a word somewhere
        for tl in TLS[A]:
            assert any(k == "escaped" for _, k in W.census(tab, A + 1, tl, 33)["shared"]), tl
    sym, s, m, w, am, b, nb, dec, _ = coded(oracle, mode, A, "nonmono")
    assert am == A and (dec != sym).any()  # the reference itself desynchronises: the expected answer is the oracle's, not y
