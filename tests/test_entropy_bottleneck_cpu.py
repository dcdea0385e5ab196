"""CPU: section 3j of include/flashgmm_amd.h - the entropy bottleneck's forward() - without a device.  The header, the export and the
binding; theta's order; the float64 restatement of tests/eb_ref.py (the arithmetic the GPU tests hold the kernels to) against the
reference's own class on the corpus (tests/golden/g11_entropy_bottleneck.npz, written by tests/golden/make_golden_eb.py); what the
corpus claims to contain; why the header deviates from the reference's written form; the module's state; refusals that need no device;
``HyperLatentCodec.forward`` over a torch stand-in of the bottleneck.  (The reference names 14 parameter tensors per bottleneck: five
matrices, five biases, four factors.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flashgmm_amd
from flashgmm_amd import EntropyBottleneck, EntropyBottleneckCoder, _lib
from flashgmm_amd.latent_codecs import HyperLatentCodec
from tests import eb_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_entropy_bottleneck.npz")))


@pytest.fixture(scope="module")
def inputs(gold):
    return torch.from_numpy(gold["x"]), {n: torch.from_numpy(gold["p." + n]) for n in R.NAMES}, torch.from_numpy(gold["med"]), torch.from_numpy(gold["g"])


def test_header_library_and_binding():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_HAS_EB 1\b", header, re.M) and " 3j. " in header
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M) and _lib.lib().fgmm_abi_version() == 6  # added without a bump
    assert int(re.search(r"^#define FGMM_EB_SLICE (\d+)\b", header, re.M).group(1)) == _lib.FGMM_EB_SLICE
    assert int(re.search(r"^#define FGMM_EB_PARAMS (\d+)\b", header, re.M).group(1)) == _lib.FGMM_EB_PARAMS == 58
    assert "MIRRORED FORM" in header  # the deviation from the reference's written form is stated where the arithmetic is
    for name, struct in (("fgmm_eb_likelihood", _lib.fgmm_eb_call), ("fgmm_eb_likelihood_backward", _lib.fgmm_eb_grad_call)):
        assert hasattr(_lib.lib(), name)
        res, args = _lib.SIGNATURES[name]  # (ctx, stream, call struct, mode, likelihood_bound)
        assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.POINTER(struct), C.c_int, C.c_float]
        # both structures begin alike: x, theta, med, B, C, hw
        assert [f[0] for f in struct._fields_[:6]] == ["x", "theta", "med", "B", "C", "hw"] and struct.hw.offset == 32
    assert C.sizeof(_lib.fgmm_eb_call) == 80 and C.sizeof(_lib.fgmm_eb_grad_call) == 88
    assert flashgmm_amd.EntropyBottleneck is EntropyBottleneck and "EntropyBottleneck" in flashgmm_amd.entropy_models.__all__


def test_theta_order():
    """M0[3] b0[3] f0[3] | M1[9] b1[3] f1[3] | M2 ... | M3 ... | M4[3] b4[1], matrices row-major [out][in]"""
    eb = EntropyBottleneck(2)
    with torch.no_grad():
        for k, n in enumerate(R.NAMES):
            p = getattr(eb, n)
            p.copy_(1000.0 * k + torch.arange(p[0].numel(), dtype=torch.float32).reshape(p[0].shape) + 0.5 * torch.arange(2.0).reshape(2, 1, 1))
    theta = eb._theta()
    assert theta.shape == (2, 58) and torch.equal(theta, R.theta_of({n: getattr(eb, n).detach() for n in R.NAMES}))
    want, layer = [], lambda k, n: [1000.0 * k + j for j in range(n)]  # noqa: E731
    for k, n in enumerate(R.NAMES):
        want += layer(k, dict(zip(R.NAMES, R.SIZES))[n])
    assert theta[0].tolist() == want and theta[1].tolist() == [v + 0.5 for v in want]
    assert R.NAMES[:3] == ("_matrix0", "_bias0", "_factor0") and R.NAMES[-2:] == ("_matrix4", "_bias4") and R.SIZES[3:6] == (9, 3, 3)
    assert theta[0, 9 + 3 * 1 + 2] == eb._matrix1[0, 1, 2]  # row-major [out][in]
    back = R.split_theta(theta.detach().numpy())
    assert all(np.array_equal(back[n], getattr(eb, n).detach().numpy()) for n in R.NAMES)


def test_restated_likelihood_equals_the_reference_in_float64(gold, inputs):
    """both forms are differences of two float64 sigmoids <= 1: an absolute bound of a few units of 2^-53"""
    x, p, med, _ = inputs
    f0 = R.forward(x, p, med, 0, dtype=torch.float64)
    f1 = R.forward(x, p, med, 1, dtype=torch.float64)
    e_L = np.abs(f0["L"].numpy() - gold["L64"]).max()
    e0, e1 = np.abs(f0["out"].numpy() - gold["like64"]).max(), np.abs(f1["out"].numpy() - gold["like64_eval"]).max()
    print(f"float64 restatement vs the reference: L {e_L:.3e}  bounded {e0:.3e}  eval {e1:.3e}")
    assert max(e_L, e0, e1) <= 4 * 2.0 ** -52
    assert np.array_equal(f1["v"].numpy(), gold["v64_eval"])
    w = R.forward(x, p, med, 0, dtype=torch.float64, mirrored=False)["L"].numpy()
    assert np.abs(w - gold["L64"]).max() <= 2.0 ** -52  # the written form restated: the class's own sequence up to the matmul's order


def test_restated_gradients_equal_the_reference_in_float64(gold, inputs):
    """relative to each tensor's largest gradient; the two forms differ by the rounding of 1 - sigmoid where it is near 0"""
    x, p, med, g = inputs
    for mode, names in ((0, [("x", "dx64")] + [(n, "d64." + n) for n in R.NAMES]), (1, [("med", "dmed64")] + [(n, "d64_eval." + n) for n in R.NAMES])):
        got = R.gradients(x, p, med, g, mode, dtype=torch.float64)
        for mine, theirs in names:
            ref = gold[theirs]
            e = np.abs(got[mine].numpy().reshape(ref.shape) - ref).max() / np.abs(ref).max()
            print(f"float64 gradient mode {mode} {mine:10s} max |g| {np.abs(ref).max():.3e}  relative error {e:.3e}")
            assert e <= 1e-12, (mode, mine, e)
    assert not R.gradients(x, p, med, g, 1, dtype=torch.float64)["x"].any() and not R.gradients(x, p, med, g, 0, dtype=torch.float64)["med"].any()


def test_corpus_has_what_it_claims(gold, inputs):
    x, p, med, g = inputs
    cx, cp, cmed, cg, cregion = R.corpus()
    assert np.array_equal(cx, gold["x"]) and np.array_equal(cg, gold["g"]) and np.array_equal(cmed, gold["med"]) and np.array_equal(cregion, gold["region"])
    assert all(np.array_equal(cp[n], gold["p." + n]) for n in R.NAMES)
    region, xs = gold["region"], gold["x"]
    for r, (lo, hi) in enumerate(((-60, 60), (-400, -60), (60, 400))):
        sel = region == r
        assert sel.any() and (xs[sel] >= lo).all() and (xs[sel] <= hi).all()
        assert (gold["g"][sel] > 0).any() and (gold["g"][sel] < 0).any()  # an upstream gradient of both signs in every region
        assert all((sel[:, c]).any() for c in range(R.C))
    f = R.forward(x, p, med, 0, dtype=torch.float64)
    flip, below = float(f["flip"].double().mean()), float((f["L"] < R.f32(R.LB)).double().mean())
    print(f"corpus: flip share {flip:.3f}, below-bound share {below:.3f}")
    assert 0.1 <= flip <= 0.9 and 0.1 <= below <= 0.9
    name, at, value = R.PLANT_MATRIX
    assert gold["p." + name][at] == value > 20  # softplus' linear branch
    name, at, value = R.PLANT_FACTOR
    assert gold["p." + name][at] == value and abs(np.tanh(value)) > 0.9


def test_written_form_is_noise_in_the_right_tail_in_binary32(gold, inputs):
    """why the header deviates: relative to max(L, 1e-9) against float64, the reference's written form is off by more than 100 times
    the mirrored form's error in the right tail - in the restatement and in the reference's own float32 run"""
    x, p, med, _ = inputs
    L64 = gold["L64"]
    den = np.maximum(L64, 1e-9)
    right = gold["region"] == 2
    err = lambda L: np.abs(L.astype(np.float64) - L64) / den  # noqa: E731
    mirrored = err(R.forward(x, p, med, 0)["L"].numpy())
    written = err(R.forward(x, p, med, 0, mirrored=False)["L"].numpy())
    theirs = err(gold["L32_written"])
    for r, name in enumerate(R.REGIONS):
        sel = gold["region"] == r
        print(f"binary32 {name:6s} mirrored {mirrored[sel].max():.3e}  written {written[sel].max():.3e}  reference's float32 {theirs[sel].max():.3e}")
    assert written[right].max() > 100 * mirrored[right].max() and theirs[right].max() > 100 * mirrored[right].max()
    assert mirrored.max() < 1e-3


def test_module_init_and_state_dict(gold):
    torch.manual_seed(3)
    eb = EntropyBottleneck(5)
    init = R.init_params(5)
    for n in R.NAMES:
        got = getattr(eb, n).detach().numpy()
        assert got.shape == init[n].shape and got.dtype == np.float32
        if "bias" in n:
            assert (np.abs(got) <= 0.5).all() and got.std() > 0.1
        else:
            assert np.array_equal(got, init[n]), n
    assert np.array_equal(eb.quantiles.detach().numpy(), np.tile(np.float32([-10, 0, 10]), (5, 1, 1)))
    t = np.log(2 / 1e-9 - 1)
    assert np.allclose(eb.target.numpy(), [-t, 0, t], rtol=1e-7) and eb.target.dtype == torch.float32
    assert eb._get_medians().shape == (5, 1, 1)
    assert all(getattr(eb, n).numel() == 0 and getattr(eb, n).dtype == torch.int32 for n in ("_offset", "_quantized_cdf", "_cdf_length"))
    # the quantile loss (entropy_models.py:429-432) in plain torch: at the initial values the logits of the outer quantiles are +-1 * ... finite
    loss = eb.loss()
    assert loss.requires_grad and torch.isfinite(loss)
    loss.backward()
    assert eb.quantiles.grad is not None and eb._matrix0.grad is None  # stop_gradient: only the quantiles learn from it
    with pytest.raises(RuntimeError, match="empty"):
        eb.coder()
    # the fixture's state dict - the reference's own module after update() - loads strictly, tables and all
    sd = {k[3:]: torch.from_numpy(v) for k, v in gold.items() if k.startswith("sd.")}
    eb = EntropyBottleneck(R.C)
    assert set(sd) == set(eb.state_dict())
    eb.load_state_dict(sd, strict=True)
    assert eb._quantized_cdf.shape == sd["_quantized_cdf"].shape and eb._quantized_cdf.numel() > 0 and torch.equal(eb._cdf_length, sd["_cdf_length"])
    assert all(torch.equal(getattr(eb, n).detach(), sd[n]) for n in R.NAMES) and torch.equal(eb._get_medians().reshape(-1), torch.from_numpy(gold["med"]))
    assert eb.likelihood_bound == float(np.float32(1e-9))
    coder = eb.coder()
    assert isinstance(coder, EntropyBottleneckCoder) and eb.coder() is coder and "_coder_cache" not in dict(eb.named_modules())
    z = torch.round(torch.from_numpy(gold["x"][:, :, :4, :4]).clamp(-30, 30))
    strings = eb.compress(z)
    assert strings == coder.compress(z) and len(strings) == 2
    assert torch.equal(eb.decompress(strings, z.shape[-2:]), torch.round(z - eb._get_medians()) + eb._get_medians())


def test_refusals_that_need_no_device():
    for filters in ((3, 3, 3), (3, 3, 3, 3, 3), (2, 3, 3, 3), ()):
        with pytest.raises(ValueError, match="filters"):
            EntropyBottleneck(4, filters=filters)
    with pytest.raises(ValueError):
        EntropyBottleneck(4, likelihood_bound=-1.0)
    eb = EntropyBottleneck(4)
    with pytest.raises(RuntimeError, match="float32"):
        eb(torch.zeros(1, 4, 2, 2, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="float32"):
        eb.rate_bits(torch.zeros(1, 4, 2, 2, dtype=torch.float16))
    with pytest.raises(RuntimeError, match=r"\[B, 4"):
        eb(torch.zeros(1, 3, 2, 2))
    with pytest.raises(RuntimeError, match="GPU"):
        eb(torch.zeros(1, 4, 2, 2))
    with pytest.raises(RuntimeError, match="empty"):
        eb.compress(torch.zeros(1, 4, 2, 2))
    # the C entry points: a null context or call structure is refused before anything is touched
    L = _lib.lib()
    call, gcall = _lib.fgmm_eb_call(), _lib.fgmm_eb_grad_call()
    assert L.fgmm_eb_likelihood(None, None, C.byref(call), 0, 1e-9) == 1 and L.fgmm_eb_likelihood_backward(None, None, C.byref(gcall), 0, 1e-9) == 1
    assert L.fgmm_eb_likelihood(None, None, None, 0, 1e-9) == 1


class _StubBottleneck(torch.nn.Module):
    """the reference's contract in plain torch: noise in training, round about the medians otherwise; a likelihood that tells the two apart"""

    def __init__(self, channels):
        super().__init__()
        self.med = torch.nn.Parameter(torch.linspace(-0.3, 0.4, channels).reshape(channels, 1, 1))

    def _get_medians(self):
        return self.med

    def forward(self, z):
        out = z + 0.25 if self.training else torch.round(z - self.med) + self.med
        return out, torch.sigmoid(out)


@pytest.mark.parametrize("quantizer", ["noise", "ste"])
def test_hyper_latent_codec_forward_with_a_stub(quantizer):
    torch.manual_seed(1)
    h_a, h_s = torch.nn.Conv2d(3, 4, 1), torch.nn.Conv2d(4, 2, 1)
    eb = _StubBottleneck(4)
    codec = HyperLatentCodec(entropy_bottleneck=eb, h_a=h_a, h_s=h_s, quantizer=quantizer)
    y = torch.randn(2, 3, 5, 5, requires_grad=True)
    for training in (True, False):
        codec.train(training)
        out = codec(y)
        z = h_a(y)
        z_hat, like = eb(z)
        if quantizer == "ste":  # hyper.py:90-92: quantize_ste about the medians, whatever the bottleneck returned
            z_hat = torch.round(z - eb.med) + eb.med
        assert set(out) == {"likelihoods", "params"} and set(out["likelihoods"]) == {"z"}
        assert torch.equal(out["likelihoods"]["z"], like) and torch.allclose(out["params"], h_s(z_hat), atol=1e-6)
    codec.eval()
    (g,) = torch.autograd.grad(codec(y)["params"].sum(), y, allow_unused=True)
    assert (g is not None and g.abs().sum() > 0) == (quantizer == "ste")  # the straight-through estimator passes the gradient to y
