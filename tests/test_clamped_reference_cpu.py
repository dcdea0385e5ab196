"""CPU: the clamped-sigma path (clamp_scales=True, what every real caller runs) of the checkers.  The corpus' guard families
(tests/edge_corpus.py CLAMP_FAMILIES) really lie on both sides of the guards they name; tests/synth.py clamps as torch.clamp does;
and the oracle equals the COMPILED reference (oracle/_ref through tests/ref_worker.py) on the clamped rows of those families and
of PARAM_FAMILIES: float CDFs, encoder bytes, both oracle decoders on valid, garbage, truncated and corrupted streams, and the
full edge table.  That is what lets tests/test_gpu_clamped_edges.py trust the reference alone and the fake device the oracle."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import edge_corpus as E
from tests import ref_worker as W
from tests import synth as T

needs_ref = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built: the reference sources were not there at build()")

MODES = ["polya", "as", "logistic"]
FAMILIES = list(E.CLAMP_FAMILIES) + list(E.PARAM_FAMILIES)
N_DEC = 512
N_TAB = 48
TAB_BS_MAX = 400


def _case(fam):
    """rows of a family, sigma PRE-clamp (PARAM_FAMILIES: symbols anywhere in int32)"""
    return E.clamp_case(fam) if fam in E.CLAMP_FAMILIES else E.param_case(fam, n=2304)


def _clamped(fam):
    c = _case(fam)
    return c["v"], E.clamp_sigma(c["s"]), c["m"], c["w"]


def _family_bs(fam):
    """max_bs of a family's decode cases: what compress would derive from its first N_DEC symbols (int32-wide ones: 200)"""
    v = _case(fam)["v"][:N_DEC].astype(np.int64)
    return int(np.abs(v).max()) + 2 if fam in E.CLAMP_FAMILIES else 200


def _streams(sf, valid):
    return ([("valid", valid)] if sf == "truncated" else []) + E.stream_cases(sf, valid, N_DEC)


# ---- the corpus -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", list(E.CLAMP_GUARDS))
def test_guard_families_lie_on_both_sides_of_their_guard(fam):
    c = E.clamp_case(fam)
    for guard in E.CLAMP_GUARDS[fam]:
        fast = guard(c).mean()
        assert 0.25 <= fast <= 0.75, (fam, guard.__name__, fast)


def test_guard_2048_lands_on_every_listed_distance():
    """(v - 0.5) - mu_k, rounded once as the kernel rounds it, equals each listed distance exactly, with both signs"""
    c = E.clamp_case("guard_2048")
    a = E._a_of(c)
    for d in E.GUARD_BELOW + E.GUARD_ABOVE:
        for sgn in (-1.0, 1.0):
            assert (a == np.float32(sgn * d)).any(), sgn * d
    hits = (np.abs(a) >= 2047).sum(1)
    assert {1, 2, 4} <= set(hits.tolist())


@pytest.mark.parametrize("fam,max_bs", [("spread_means", 3001), ("spread_means_1022", E.SEGDEC_AM), ("spread_means_510", 510)])
def test_spread_means_rows_mix_fast_and_slow_pairs(fam, max_bs):
    c = E.clamp_case(fam)
    assert int(np.abs(c["v"].astype(np.int64)).max()) + 1 == max_bs
    fast, slow = E.window_pair_kinds(c, max_bs)
    assert ((fast >= 4) & (slow >= 4)).mean() >= 0.25
    apart = c["m"].max(1) - c["m"].min(1)
    assert (apart > 2048).all() and (apart < 4096).all()
    if fam == "spread_means":
        assert (np.abs(c["m"]) <= max_bs).all()
    else:
        assert 2 * (max_bs + 1) + 2 <= 2048 and (c["m"].min(1) < -max_bs - 1).all() and (c["m"].max(1) > max_bs + 1).all()


def test_the_other_families_hold_what_they_promise():
    c = E.clamp_case("nan_sigma_one")
    assert set(np.isnan(c["s"]).sum(1).tolist()) == {0, 1, 2, 3, 4}
    c = E.clamp_case("sigma_at_clamp")
    for val in E.SIGMA_AT_CLAMP:
        assert (c["s"].view(np.uint32) == val.view(np.uint32)).any(), val
    c = E.clamp_case("sat_edges")
    assert E.near_sat_edge(c, 41).mean() >= 0.25
    assert E.near_sat_edge({**c, "s": np.full_like(c["s"], 1.0), "m": c["m"] + np.float32(0.37)}, 41).mean() < 0.05
    c = E.clamp_case("logistic_rcp_guard")
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (E._a_of(c) / E.clamp_sigma(c["s"])).astype(np.float32)
    zt = np.float32(-60.0 * np.log(2.0) / 1.702)
    assert len(np.unique(z[np.abs(z - zt) <= 64 * np.spacing(-zt)])) >= 100  # the band of single ulps around the threshold
    assert z.min() < -2000 / 0.11
    w = E.clamp_case("window_weights")["w"]
    s = ((w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])).astype(np.float32)
    with np.errstate(invalid="ignore"):
        assert (s * np.float32(65535) >= 65536).any() and (s < 1).any() and (w == 0).all(1).any()
        assert (w == np.nextafter(np.float32(1), np.float32(2))).any() and np.isnan(w).any() and np.isinf(w).any()
        assert ((w == 0) & np.signbit(w)).any() and ((w < 0) & (w > -1e-7)).any()
    for fam in E.CLAMP_FAMILIES:
        assert int(np.abs(E.clamp_case(fam)["v"].astype(np.int64)).max()) + 2 <= 40000  # every decoder takes the item


@pytest.mark.parametrize("fam", FAMILIES)
def test_synth_clamps_as_torch_clamp(fam):
    """synth.to_coder_inputs(clamp=True) against torch.clamp(s, 0.11, 256), bit for bit: NaN kept, -0 / -inf -> 0.11, +inf -> 256"""
    c = _case(fam)
    n = len(c["v"])
    M, hw = 9, n // 9

    def planes(a):
        return np.ascontiguousarray(a.reshape(M, hw, 4).transpose(2, 0, 1).reshape(1, 4 * M, hw, 1))

    y = np.ones((1, M, hw, 1), np.float32)
    _, s, m, w, *_ = T.to_coder_inputs(y, planes(c["s"]), planes(c["m"]), planes(c["w"]), clamp=True)
    want = torch.clamp(torch.from_numpy(c["s"]), 0.11, 256).numpy()
    assert np.array_equal(np.ascontiguousarray(s).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(E.clamp_sigma(c["s"]).view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.isnan(want), np.isnan(c["s"]))
    assert np.array_equal(np.ascontiguousarray(m).view(np.uint32), c["m"].view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(w).view(np.uint32), c["w"].view(np.uint32))
    if fam == "sigma_at_clamp":
        got = {np.float32(a).tobytes(): b for a, b in zip(c["s"].reshape(-1), want.reshape(-1))}
        for a, b in ((-0.0, 0.11), (0.0, 0.11), (-np.inf, 0.11), (-1.5, 0.11), (1e-40, 0.11), (np.inf, 256), (3.4028235e38, 256)):
            assert got[np.float32(a).tobytes()] == np.float32(b), a


# ---- the oracle against the compiled reference ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cases(mode):
    cases = {}
    for fam in FAMILIES:
        v, s, m, w = _clamped(fam)
        x1, x2 = E.abscissae_for(E._rng("clamp/x/" + fam), len(v))
        cases[f"{fam}.cdf"] = {"kind": "cdf", "v": v, "s": s, "m": m, "w": w}
        cases[f"{fam}.cdfx"] = {"kind": "cdf_x", "x1": x1, "x2": x2, "s": s, "m": m, "w": w}
        cases[f"{fam}.enc"] = {"kind": "encode", "v": v, "s": s, "m": m, "w": w}
        sd, md, wd = (np.ascontiguousarray(a[:N_DEC]) for a in (s, m, w))
        valid = O.encode_gmm(mode, v[:N_DEC], sd, md, wd)
        for sf in E.STREAM_FAMILIES:
            for tag, b in _streams(sf, valid):
                for bs in (37, _family_bs(fam)):
                    cases[f"{fam}.{sf}.{tag}.{bs}"] = {"kind": "decode", "bytes": np.frombuffer(b, np.uint8), "s": sd, "m": md,
                                                       "w": wd, "max_bs": np.int32(bs)}
        # the full edge table of the first N_TAB rows: every edge v - 0.5, v in [-max_bs, max_bs + 1], as a cdf_x abscissa
        bs = _family_bs(fam)
        x = (np.arange(-bs, bs + 2).astype(np.float32) - np.float32(0.5)).astype(np.float32)
        rep = lambda a: np.ascontiguousarray(np.repeat(a[:N_TAB], len(x), 0))  # noqa: E731
        cases[f"{fam}.tab"] = {"kind": "cdf_x", "x1": np.tile(x, N_TAB), "x2": np.tile(x, N_TAB), "s": rep(s), "m": rep(m), "w": rep(w)}
    return cases


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    got = {}

    def get(mode):
        if mode not in got:
            got[mode] = W.run(mode, _cases(mode), tmp_path_factory.mktemp(f"ref_{mode}"))
        return got[mode]

    return get


def _differ(got, want):
    """bit for bit, except that a NaN equals any NaN (tests/test_gpu_reference_edges.py: _differ)"""
    g, w = (np.ascontiguousarray(a, np.float32) for a in (got, want))
    return (g.view(np.uint32) != w.view(np.uint32)) & ~(np.isnan(g) & np.isnan(w))


def quant16(c):
    """static_cast<uint16_t>(cdf * 65535) as x86-64 compiles it (cvttss2si, low 16 bits): the oracle's fgo_u16"""
    with np.errstate(invalid="ignore", over="ignore"):
        return (T.torch_int((np.asarray(c, np.float32) * np.float32(65535)).astype(np.float32)).astype(np.int64) & 0xFFFF).astype(np.uint16)


@needs_ref
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_float_cdf_equals_compiled_reference(ref, mode, fam):
    r, c = ref(mode), _cases(mode)
    for kind in ("cdf", "cdfx"):
        x, want = c[f"{fam}.{kind}"], r[f"{fam}.{kind}"]
        if kind == "cdf":
            c1, c2 = O.gmm_cdf(mode, x["v"], x["s"], x["m"], x["w"])
        else:
            c1, c2 = O.gmm_cdf_x(mode, x["x1"], x["x2"], x["s"], x["m"], x["w"])
        bad = np.nonzero(_differ(c1, want["c1"]) | _differ(c2, want["c2"]))[0]
        assert len(bad) == 0, (kind, len(bad), bad[:5])


@needs_ref
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_encode_equals_compiled_reference(ref, mode, fam):
    x = _cases(mode)[f"{fam}.enc"]
    got = O.encode_gmm(mode, x["v"], x["s"], x["m"], x["w"])
    assert got == ref(mode)[f"{fam}.enc"]["bytes"].tobytes()
    assert O.rans_encode_symtab(O.symtab(mode, x["v"], x["s"], x["m"], x["w"]), x["v"]) == got


def _agree(decode, want, what):
    """tests/test_reference_edges_cpu.py: _agree"""
    try:
        got = decode()
    except RuntimeError:
        assert int(want["past_end"]) == 1, f"{what}: the oracle refused a stream the reference decodes within its bytes"
        return 0
    assert np.array_equal(got, want["syms"]), (what, np.nonzero(got != want["syms"])[0][:5])
    return 1


@needs_ref
@pytest.mark.parametrize("sf", E.STREAM_FAMILIES)
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_decode_equals_compiled_reference(ref, mode, fam, sf):
    """decode_gmm (float bisection) and, up to max_bs 400, the integer decode from the full edge table, on the valid stream
    and on garbage, truncated and corrupted ones"""
    r, c = ref(mode), _cases(mode)
    valid = O.encode_gmm(mode, *(c[f"{fam}.enc"][k][:N_DEC] for k in ("v", "s", "m", "w")))
    answered = 0
    for tag, b in _streams(sf, valid):
        for bs in (37, _family_bs(fam)):
            name = f"{fam}.{sf}.{tag}.{bs}"
            x, want = c[name], r[name]
            answered += _agree(lambda: O.decode_gmm(mode, b, x["s"], x["m"], x["w"], bs), want, name)
            if bs <= TAB_BS_MAX:
                tab = O.cdftab(mode, x["s"], x["m"], x["w"], bs)
                _agree(lambda: O.rans_decode_cdftab(b, tab, bs), want, name + " (cdftab)")
    # (a family with weights that are no distribution need not decode, not even from its own stream: the oracle may refuse all)
    assert answered > 0 or sf == "flipped" or fam in E.CLAMP_NONMONO_FAMILIES


@needs_ref
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("mode", MODES)
def test_cdftab_equals_the_table_of_the_compiled_reference(ref, mode, fam):
    """oracle.cdftab on clamped rows, entry for entry, against the reference's _fast_gmm_cdf<4> at every edge v - 0.5 quantised
    as the coder quantises (quant16 above; the conversion itself is pinned by the encoder tests)"""
    bs = _family_bs(fam)
    x = _cases(mode)[f"{fam}.enc"]
    got = O.cdftab(mode, *(np.ascontiguousarray(x[k][:N_TAB]) for k in ("s", "m", "w")), bs)
    want = quant16(ref(mode)[f"{fam}.tab"]["c1"]).reshape(N_TAB, 2 * bs + 2)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
