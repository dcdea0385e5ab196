"""CPU: the oracle (oracle/fgmm_oracle.c) against the COMPILED reference (oracle/_ref, run by tests/ref_worker.py) on the edge
corpus of tests/edge_corpus.py - so that the oracle, which every other edge-case test trusts, is itself checked where it is
most likely to be wrong: non-finite and degenerate parameters, symbols anywhere in int32, garbage / truncated / corrupted
streams, and the latent quantisation of tests/synth.py against torch's own ops."""
import functools

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import edge_corpus as E
from tests import ref_worker as W
from tests import synth as T

pytestmark = pytest.mark.skipif(not O.ref_available(), reason="oracle/_ref not built: the reference sources were not there at build()")

MODES = ["polya", "as", "logistic"]
N_DEC = 512
DEC_BS = (5, 37, 127, 200, 3000)
TAB_BS_MAX = 400


def _streams(fam, valid):
    return ([("valid", valid)] if fam == "truncated" else []) + E.stream_cases(fam, valid, N_DEC)


def _rows(c, k=None):
    sl = slice(0, k)
    return [np.ascontiguousarray(c[f][sl]) for f in ("s", "m", "w")]


def _latent_inputs(y, s, m, w):
    sym, s2, m2, w2, am, zb, yq = T.to_coder_inputs(y, s, m, w)
    return sym, [np.ascontiguousarray(a, np.float32) for a in (s2, m2, w2)], am, zb, yq


@functools.lru_cache(maxsize=None)
def _cases(mode):
    """every case of one mode: name -> inputs (what the worker is given)"""
    cases = {}
    for fam in E.PARAM_FAMILIES:
        c = E.param_case(fam)
        s, m, w = _rows(c)
        cases[f"{fam}.cdf"] = {"kind": "cdf", "v": c["v"], "s": s, "m": m, "w": w}
        cases[f"{fam}.cdfx"] = {"kind": "cdf_x", "x1": c["x1"], "x2": c["x2"], "s": s, "m": m, "w": w}
        cases[f"{fam}.enc"] = {"kind": "encode", "v": c["v"], "s": s, "m": m, "w": w}
        sd, md, wd = _rows(c, N_DEC)
        valid = O.encode_gmm(mode, c["v"][:N_DEC], sd, md, wd)
        for sf in E.STREAM_FAMILIES:
            for tag, b in _streams(sf, valid):
                for bs in DEC_BS:
                    cases[f"{fam}.{sf}.{tag}.{bs}"] = {"kind": "decode", "bytes": np.frombuffer(b, np.uint8), "s": sd, "m": md,
                                                       "w": wd, "max_bs": np.int32(bs)}
    for fam in E.LATENT_FAMILIES:
        sym, (s, m, w), *_ = _latent_inputs(*E.latent_case(fam))
        cases[f"lat_{fam}.enc"] = {"kind": "encode", "v": sym, "s": s, "m": m, "w": w}
    for fam in E.FP16_FAMILIES:
        y, s16, m16, w16 = E.fp16_case(fam)
        sym, (s, m, w), *_ = _latent_inputs(y, *(a.astype(np.float32) for a in (s16, m16, w16)))
        cases[f"{fam}.enc"] = {"kind": "encode", "v": sym, "s": s, "m": m, "w": w}
    if mode == MODES[0]:
        for name, p in E.PMF_CASES.items():
            cases[f"pmf_{name}"] = {"kind": "pmf", "pmf": np.asarray(p, np.float32)}
    return cases


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    got = {}

    def get(mode):
        if mode not in got:
            got[mode] = W.run(mode, _cases(mode), tmp_path_factory.mktemp(f"ref_{mode}"))
        return got[mode]

    return get


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("fam", list(E.PARAM_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_float_cdf_equals_compiled_reference(ref, mode, fam):
    r, c = ref(mode), _cases(mode)
    for kind in ("cdf", "cdfx"):
        x = c[f"{fam}.{kind}"]
        if kind == "cdf":
            c1, c2 = O.gmm_cdf(mode, x["v"], x["s"], x["m"], x["w"])
        else:
            c1, c2 = O.gmm_cdf_x(mode, x["x1"], x["x2"], x["s"], x["m"], x["w"])
        want = r[f"{fam}.{kind}"]
        bad = np.nonzero((_bits(c1) != _bits(want["c1"])) | (_bits(c2) != _bits(want["c2"])))[0]
        assert len(bad) == 0, (kind, len(bad), bad[:5])


@pytest.mark.parametrize("fam", list(E.PARAM_FAMILIES) + [f"lat_{f}" for f in E.LATENT_FAMILIES] + list(E.FP16_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_encode_equals_compiled_reference(ref, mode, fam):
    """symtab -> rANS bytes (encode_gmm) against RansEncoder.encode_with_indexes_gmm"""
    x = _cases(mode)[f"{fam}.enc"]
    got = O.encode_gmm(mode, x["v"], x["s"], x["m"], x["w"])
    assert got == ref(mode)[f"{fam}.enc"]["bytes"].tobytes()
    if fam in E.PARAM_FAMILIES:  # the same through the oracle's symbol table and its table-driven coder
        assert O.rans_encode_symtab(O.symtab(mode, x["v"], x["s"], x["m"], x["w"]), x["v"]) == got


def _agree(decode, want, what):
    """the oracle's decoder reads zero words past the end of the stream (a few), then refuses: where it answers, the answer is
    the reference's on the zero-padded stream; where it refuses, the reference must have depended on words past the end"""
    try:
        got = decode()
    except RuntimeError:
        assert int(want["past_end"]) == 1, f"{what}: the oracle refused a stream the reference decodes within its bytes"
        return 0
    assert np.array_equal(got, want["syms"]), (what, np.nonzero(got != want["syms"])[0][:5])
    return 1


@pytest.mark.parametrize("sf", E.STREAM_FAMILIES)
@pytest.mark.parametrize("fam", list(E.PARAM_FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_decode_equals_compiled_reference(ref, mode, fam, sf):
    """decode_gmm (float bisection) and, for max_bs <= 400, the integer decode from the full edge table (cdftab), against
    RansDecoder.decode_with_indexes_gmm on garbage, truncated and corrupted streams"""
    r, c = ref(mode), _cases(mode)
    valid = O.encode_gmm(mode, *(c[f"{fam}.enc"][k][:N_DEC] for k in ("v", "s", "m", "w")))
    answered = 0
    for tag, b in _streams(sf, valid):
        for bs in DEC_BS:
            name = f"{fam}.{sf}.{tag}.{bs}"
            x, want = c[name], r[name]
            answered += _agree(lambda: O.decode_gmm(mode, b, x["s"], x["m"], x["w"], bs), want, name)
            if bs <= TAB_BS_MAX:
                tab = O.cdftab(mode, x["s"], x["m"], x["w"], bs)
                _agree(lambda: O.rans_decode_cdftab(b, tab, bs), want, name + " (cdftab)")
    assert answered > 0


@pytest.mark.parametrize("fam", list(E.LATENT_FAMILIES) + list(E.FP16_FAMILIES))
def test_latent_quantisation_equals_torch(fam):
    """tests/synth.py:to_coder_inputs against the reference's own lines (entropy_models.py:834-846) as torch CPU ops: abs_max
    (torch.max / torch.min keep NaN, .int() of NaN / inf / |y| >= 2^31 is INT32_MIN), zero_bitmap, the symbols, y_q"""
    if fam in E.LATENT_FAMILIES:
        y, s, m, w = E.latent_case(fam)
    else:
        y, s, m, w = (a.astype(np.float32) for a in E.fp16_case(fam))
    sym, _, am, zb, yq = _latent_inputs(y, s, m, w)
    yt = torch.from_numpy(y)
    am_ref = max(torch.abs(yt.max()).int().item(), torch.abs(yt.min()).int().item()) + 1
    am_ref = 1 if am_ref < 1 else am_ref
    yq_ref = torch.round(yt)
    zb_ref = torch.where(torch.sum(torch.abs(yq_ref), (3, 2)).squeeze(0) == 0, 0, 1)
    nonzero = torch.nonzero(zb_ref).flatten().tolist()
    sym_ref = yq_ref[:, nonzero].reshape(-1).int()
    assert am == am_ref
    assert zb.tolist() == zb_ref.tolist()
    assert np.array_equal(sym, sym_ref.numpy())
    assert np.array_equal(yq, yq_ref.numpy(), equal_nan=True)
    if fam == "one_nan":
        assert am == 1  # the NaN makes y.max() NaN: .int() -> INT32_MIN, floored at 1


@pytest.mark.parametrize("name", list(E.PMF_CASES))
def test_pmf_to_quantized_cdf_equals_compiled_reference(ref, name):
    """the oracle's and the product's pmf_to_quantized_cdf against compressai._CXX on degenerate pmfs"""
    from flashgmm_amd import ops

    want = ref(MODES[0])[f"pmf_{name}"]
    pmf = E.PMF_CASES[name]
    for fn in (O.pmf_to_quantized_cdf, ops.pmf_to_quantized_cdf):
        if int(want["error"]):
            with pytest.raises(ValueError):
                fn(pmf, 16)
        else:
            assert fn(pmf, 16) == want["cdf"].tolist()
