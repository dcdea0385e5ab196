"""CPU: the parameter head's checker and the bounds the GPU tests hold its kernels to (tests/head_ref.py), on the head families of
tests/edge_corpus.py.

  - oracle.head_params (the fmaf chain the f32 kernel must equal bit for bit) is within the rigorous chain bound of a float64 reference
    on every finite family, and has float64's IEEE class (finite, +inf, -inf, NaN) on the non-finite ones
  - the numpy split3 is fgmm_head16.hip's: exact for normal values, within 2^-134 below the bfloat16 normal range; from it, the
    bf16x6 bound - an emulation of the kernel's arithmetic (six part products, one binary32 rounding per matrix step) stays inside it
  - the identity head of the fused tests reproduces any finite plane through the chain bit for bit, -0 excepted (it comes out +0)"""
import numpy as np
import pytest

from tests import edge_corpus as E
from tests import head_ref as H

F32 = np.float32
SHAPES = [(1, 1, 1), (15, 17, 33), (17, 33, 65), (16, 64, 4), (2, 1040, 3)]
FINITE = [f for f in E.HEAD_FAMILIES if f not in E.HEAD_NONFINITE]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fam", FINITE)
def test_oracle_chain_within_the_float64_bound(oracle, fam, shape):
    W, b, x = E.head_case(fam, *shape)
    got = oracle.head_params(W, b, x).astype(np.float64)
    want, bound = H.exact(W, b, x), H.chain_bound(W, b, x)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    err = np.abs(got - want)
    assert (err <= bound).all(), (fam, shape, float((err / bound).max()))
    if fam == "cancellation":  # the family does what it says: results far below sum |w x|
        assert (np.abs(want[:, 0]) < 1e-3 * H.abs_sum(W, b, x)[:, 0]).mean() > 0.9
    if fam == "tiny_products" and shape[1] * shape[2] >= 16:  # products below the normal range, where every rounding is an absolute 2^-150 at most
        assert float(np.abs(W).min()) * float(np.abs(x).min()) < 2.0**-126


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fam", E.HEAD_NONFINITE)
def test_oracle_chain_has_the_ieee_class_of_float64(oracle, fam, shape):
    """the class of b + sum w x does not depend on the summation order as long as no finite partial sum overflows (the finite
    parts of these families are ordinary): NaN iff a NaN term or +inf and -inf terms, else +-inf iff an infinite term"""
    W, b, x = E.head_case(fam, *shape)
    got = oracle.head_params(W, b, x)
    want = H.exact(W, b, x)
    assert (H.ieee_class(want) != 0).any()
    assert np.array_equal(H.ieee_class(got), H.ieee_class(want)), fam


def _values(rng, n):
    """binary32 values over the whole range: normal, subnormal, near the bfloat16 overflow, zeros"""
    v = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * np.exp2(rng.uniform(-149, 127.99, n))).astype(F32)
    v[:8] = [0.0, -0.0, 2.0**-149, -(2.0**-126), 1.0, float.fromhex("0x1.FEFFFEp127"), 2.0**-110, 1.0 + 2.0**-23]
    return v


def test_split3_is_exact_for_normal_values_and_within_half_a_subnormal_below():
    v = _values(np.random.default_rng(1), 400000)
    v = v[np.abs(v) < E.BF16_OVERFLOW]
    a, b, c = H.split3(v)
    for p in (a, b, c):  # every part a bfloat16
        assert np.array_equal(H.to_bf16(p).view(np.uint32), p.view(np.uint32))
    s = a.astype(np.float64) + b + c
    err = np.abs(s - v.astype(np.float64))
    v3_normal = (np.abs(c) >= 2.0**-126) | (c == 0) & (np.abs(v) >= 2.0**-110)
    assert (err[np.abs(v) >= 2.0**-110] == 0).all() and (err[v3_normal] == 0).all()
    assert (err <= 2.0**-134).all()
    av = np.abs(v.astype(np.float64))
    assert (np.abs(b) <= 2.0**-8 * (1 + 2.0**-8) * av + 2.0**-133).all()
    assert (np.abs(c) <= 2.0**-16 * (1 + 2.0**-7) * av + 2.0**-133).all()
    # round to nearest even, and the bfloat16 overflow point
    assert H.to_bf16(np.array([1 + 2.0**-8], F32))[0] == 1.0 and H.to_bf16(np.array([1 + 3 * 2.0**-8], F32))[0] == 1 + 2.0**-6
    assert np.isinf(H.to_bf16(np.array([E.BF16_OVERFLOW], F32))[0])
    assert np.isfinite(H.to_bf16(np.nextafter(np.array([E.BF16_OVERFLOW], F32), F32(0)))[0])
    assert np.isnan(H.split3(np.array([np.inf], F32))[1][0])  # inf - inf: the reason non-finite features leave the bf16x6 kernels


def test_split3_dropped_products_and_residuals_within_the_derived_terms():
    rng = np.random.default_rng(2)
    w, x = _values(rng, 300000), _values(rng, 300000)
    ok = (np.abs(w) < 2.0**63) & (np.abs(x) < 2.0**63)
    w, x = w[ok], x[ok]
    (w1, w2, w3), (x1, x2, x3) = H.split3(w), H.split3(x)
    d = lambda a: a.astype(np.float64)  # noqa: E731
    kept = d(w1) * d(x3) + d(w3) * d(x1) + d(w2) * d(x2) + d(w1) * d(x2) + d(w2) * d(x1) + d(w1) * d(x1)
    err = np.abs(kept - d(w) * d(x))
    assert (err <= 2.0**-23 * (1 + 2.0**-6) * np.abs(d(w) * d(x)) + 2.0**-133 * (np.abs(d(w)) + np.abs(d(x)))).all()


def _emulate_bf16x6(W, b, x):
    """fgmm_head16.hip's arithmetic on the CPU under the bound's model: per 16 input channels, six steps (part products smallest
    first), each adding the step's exact sum of products to the binary32 accumulator with one rounding"""
    Ws, xs = H.split3(W), H.split3(x)
    acc = np.zeros((W.shape[0], x.shape[1]), F32) + (b[:, None] if b is not None else F32(0))
    order = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))
    for k0 in range(0, W.shape[1], 16):
        for qa, qb in order:
            step = Ws[qa][:, k0:k0 + 16].astype(np.float64) @ xs[qb][k0:k0 + 16].astype(np.float64)
            acc = (acc.astype(np.float64) + step).astype(F32)
    return acc


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("fam", [f for f in FINITE if f not in E.HEAD_BF16_FEATURES_OUT])
def test_bf16x6_bound_covers_the_emulated_arithmetic(fam, shape):
    W, b, x = E.head_case(fam, *shape)
    got = _emulate_bf16x6(W, b, x).astype(np.float64)
    err, bound = np.abs(got - H.exact(W, b, x)), H.bf16x6_bound(W, b, x)
    assert (err <= bound).all(), (fam, shape, float((err / bound).max()))
    # ... and the bound is tight enough to see one part dropped (the third part of every feature zeroed) at small c_in
    if fam == "ordinary" and shape[1] <= 33 and shape[2] >= 33:
        Ws, xs = H.split3(W), H.split3(x)
        lost = np.abs(Ws[0].astype(np.float64) @ xs[2].astype(np.float64))
        assert (lost > bound).any()


@pytest.mark.parametrize("fam", ["ordinary", "wide_range", "huge", "subnormal", "tiny_products", "signed_zeros", "dead_rows"])
def test_identity_head_reproduces_finite_planes_except_negative_zero(oracle, fam):
    """the fused tests feed a head W = I (c_in = 12 M, no bias) the parameter planes: the chain gives them back bit for bit, but a
    -0 becomes +0 (the chain starts at the +0 of no bias; +0 + -0 = +0)"""
    M = 2
    _, _, x = E.head_case(fam, M, 12 * M, 37)
    x[3, :5] = [-0.0, 0.0, -0.0, float.fromhex("0x1p-149"), -3.4028235e38]
    W, b = H.identity_head(M)
    got = oracle.head_params(W, b, x)
    want = np.where((x == 0), F32(0.0), x).astype(F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
