"""GPU: section 3k of include/flashgmm_amd.h - the entropy bottleneck's update(): ``eb_quantile_kernel`` and ``eb_pmf_kernel`` behind
``fgmm_eb_quantiles`` / ``fgmm_eb_tables``, and ``EntropyBottleneck.update`` over them - against ``eb_kernel`` (the masses are its
likelihoods, bit for bit), against the float64 restatement of tests/eb_update_ref.py by the project's rule (E_k <= 2 * E_ref + 2^-23,
E_ref torch's float32 mirrored form on the same GPU, relative with floor 2^-17), and against the reference's own class through the
fixtures g11 / g12.  The decided-entry rule for tables is stated in tests/test_eb_update_cpu.py; here the masses a table was quantised
from are at hand (``pmf_out``), so the rule is applied to their counts, however many entries are undecided.

The corpus (tests/eb_update_ref.py): seven channels, rows of 322, 28, 213, 268, 140, 1023 and 2 entries with their tails - none a multiple
of a wave, the longest over four workgroups, the shortest a single mass.

Measured on one MI355X (profiles/eb_update.md): E_k equals E_ref in every channel (1.2e-6 to 6.0e-5 for the masses), tau = 1.202e-4, 2 to
19 undecided entries per channel, none rounded the other way by the kernel - all seven tables equal the float64 restatement's; quantiles
within 7.6e-5 of the float64 bisection."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import flashgmm_amd
from flashgmm_amd import EntropyBottleneck, EntropyBottleneckCoder, _lib, ops
from test_gpu_streams import delay, pending, snapshot, streams  # noqa: F401  (the stream case runs in that module's manner, on its helpers)
from tests import eb_ref as R
from tests import eb_update_ref as U
from tests import synth as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4
GUARDVAL = -777.25
HOST_FILL = -5


def dv(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Guarded:
    """a float32 device buffer of n elements pre-filled with NaN, between guard elements"""

    def __init__(self, n):
        self.n, self.raw = n, torch.full((n + 2 * GUARD,), GUARDVAL, dtype=torch.float32, device=DEV)
        self.t = self.raw[GUARD:GUARD + n]
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.raw[:GUARD] == GUARDVAL).all() and (self.raw[GUARD + self.n:] == GUARDVAL).all())

    def untouched(self):
        return self.intact() and bool(torch.isnan(self.t).all())


def raw_tables(theta, start, length, stride, pmf=True):
    """fgmm_eb_tables -> (rc, pmf [C, stride] or None, cdf int32 [C, stride + 1] (host), failed channel, guards intact)"""
    Cn = theta.shape[0]
    g = Guarded(Cn * stride) if pmf else None
    host = np.full(Cn * (stride + 1) + 2 * GUARD, HOST_FILL, np.int32)
    failed = C.c_int32(-7)
    rc = _lib.lib().fgmm_eb_tables(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, theta.data_ptr(), start.data_ptr(), length.data_ptr(), Cn, stride,
                                   g.t.data_ptr() if g else None, host[GUARD:].ctypes.data, C.byref(failed))
    intact = (g is None or g.intact()) and (host[:GUARD] == HOST_FILL).all() and (host[-GUARD:] == HOST_FILL).all()
    return rc, (g.t.reshape(Cn, stride) if g else None), host[GUARD:-GUARD].reshape(Cn, stride + 1), failed.value, bool(intact)


def raw_quantiles(theta, tgt=None, radius=U.SEARCH_RADIUS):
    """fgmm_eb_quantiles -> (rc, q [C, 3] device, guards intact); stream-ordered: the caller synchronises before it looks"""
    Cn = theta.shape[0]
    g = Guarded(Cn * 3)
    tg = (C.c_float * 3)(*(U.targets() if tgt is None else tgt).tolist())
    rc = _lib.lib().fgmm_eb_quantiles(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, theta.data_ptr(), Cn, tg, radius, g.t.data_ptr())
    return rc, g.t.reshape(Cn, 3), g


def eb_kernel_map(theta, x):
    """fgmm_eb_likelihood, mode 0, no bound, on x [C, n] -> its map [C, n]"""
    Cn, n = x.shape
    x3 = x.reshape(1, Cn, n).contiguous()
    like, med = torch.full_like(x3, float("nan")), torch.zeros(Cn, device=DEV)
    call = _lib.fgmm_eb_call(x3.data_ptr(), theta.data_ptr(), med.data_ptr(), 1, Cn, n, like.data_ptr(), None, None, None, 0, 0)
    torch.cuda.current_stream().synchronize()
    assert _lib.lib().fgmm_eb_likelihood(_lib.ctx(0), torch.cuda.current_stream().cuda_stream, C.byref(call), 0, 0.0) == 0
    return like[0]


@pytest.fixture(scope="module")
def g11():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_entropy_bottleneck.npz")))


@pytest.fixture(scope="module")
def corpus():
    """computed once, left unchanged: the corpus on the GPU, one raw call on it, torch's float32 mirrored form there and the float64 restatement"""
    co = U.corpus()
    offset, start, length = U.support(co["q32"])
    theta, stride = co["theta"].to(DEV), int(length.max()) + 1
    rc, pmf, cdf, failed, intact = raw_tables(theta, dv(start), dv(length), stride)
    ref32 = U.masses(co["params"], start, length, torch.float32, device=DEV)
    u64 = U.update(co["params"], co["q32"], torch.float64)
    e_ref = max(U.e_rel(ref32[0], u64["pmf"]), U.e_rel(ref32[1], u64["tail"]))
    return dict(co=co, offset=offset, start=start, length=length, theta=theta, stride=stride, rc=rc, pmf=pmf, cdf=cdf, failed=failed, intact=intact,
                ref32=ref32, u64=u64, e_ref=e_ref, tau=2 * e_ref + 2.0 ** -23)


# ---- a. the masses ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 37])
def test_masses_are_eb_kernels_likelihoods_bit_for_bit(corpus, extra):
    """entries i < length: the map eb_kernel writes for x = start + i (mode 0, bound 0); after the tail: +0; nothing outside the rows"""
    start, length, stride = corpus["start"], corpus["length"], corpus["stride"] + extra
    rc, pmf, cdf, failed, intact = raw_tables(corpus["theta"], dv(start), dv(length), stride)
    assert rc == 0 and failed == -1 and intact
    like = eb_kernel_map(corpus["theta"], dv(U.samples(start, length)))
    bits, want = pmf.view(torch.int32).cpu().numpy(), like.view(torch.int32).cpu().numpy()
    for c, n in enumerate(length.tolist()):
        assert np.array_equal(bits[c, :n], want[c, :n]), c
        assert not bits[c, n + 1:].any() and bits[c, n] != 0  # +0 after the tail, which is there
        assert not cdf[c, n + 2:].any() and cdf[c, 0] == 0 and cdf[c, n + 1] == 65536 and (np.diff(cdf[c, :n + 2]) > 0).all()
    assert torch.equal(pmf[:, :corpus["stride"]], corpus["pmf"]) and np.array_equal(cdf[:, :corpus["stride"] + 1], corpus["cdf"])  # whatever the stride


def test_masses_and_tail_against_float64(corpus):
    assert corpus["rc"] == 0 and corpus["intact"]
    got, u64, (ref_pmf, ref_tail) = corpus["pmf"].cpu().numpy(), corpus["u64"], corpus["ref32"]
    for c, n in enumerate(corpus["length"].tolist()):
        e_ref, e_k = U.e_rel(ref_pmf[c, :n], u64["pmf"][c, :n]), U.e_rel(got[c, :n], u64["pmf"][c, :n])
        t_ref, t_k = U.e_rel(ref_tail[c], u64["tail"][c]), U.e_rel(got[c, n], u64["tail"][c])
        print(f"channel {c} ({n:4d} masses)  E_ref {e_ref:.3e}  E_k {e_k:.3e}   tail {u64['tail'][c]:.6e}: E_ref {t_ref:.3e}  E_k {t_k:.3e}")
        assert e_k <= 2 * e_ref + 2.0 ** -23 and t_k <= 2 * t_ref + 2.0 ** -23
    assert (got[:6, corpus["length"][:6]].diagonal() < U.TAIL_MASS).all()


# ---- b. the tables ------------------------------------------------------------------------------------------------------------------------
def test_tables_are_the_quantiser_on_the_returned_masses(corpus):
    pmf, cdf = corpus["pmf"].cpu().numpy(), corpus["cdf"]
    assert cdf.dtype == np.int32 and cdf.shape == (U.C7, corpus["stride"] + 1)
    for c, n in enumerate(corpus["length"].tolist()):
        assert cdf[c, :n + 2].tolist() == ops.pmf_to_quantized_cdf(pmf[c, :n + 1], 16) and not cdf[c, n + 2:].any()
    rc, none, cdf2, failed, intact = raw_tables(corpus["theta"], dv(corpus["start"]), dv(corpus["length"]), corpus["stride"], pmf=False)
    assert rc == 0 and none is None and intact and np.array_equal(cdf2, cdf)  # pmf_out is optional; the same call gives the same tables


def test_tables_against_the_float64_restatement(corpus):
    """the decided-entry rule on the counts of the returned masses (and the test above: the table is the quantiser's function of them)"""
    pmf, u64, tau = corpus["pmf"].cpu().numpy(), corpus["u64"], corpus["tau"]
    print(f"E_ref {corpus['e_ref']:.3e}  tau {tau:.3e}")
    for c, n in enumerate(corpus["length"].tolist()):
        prob64 = U.entries(u64["pmf"], u64["tail"], u64["length"], c)
        ok, idx, off = U.counts_admissible(pmf[c, :n + 1], prob64, tau)
        same = np.array_equal(corpus["cdf"][c, :n + 2], u64["cdf"][c, :n + 2])
        print(f"channel {c}: {len(idx)} undecided of {n + 1}, the kernel rounds {off} the other way; table equal to the float64 one: {same}")
        assert ok and (same or off)
        if not idx:
            assert same


# ---- c. the quantiles ---------------------------------------------------------------------------------------------------------------------
def test_quantiles(corpus):
    theta, co = corpus["theta"], corpus["co"]
    rc, q, g = raw_quantiles(theta)
    torch.cuda.synchronize()
    assert rc == 0 and g.intact()
    got, ref = q.cpu().numpy()[:6].astype(np.float64), co["q64"][:6]
    d = np.abs(got - ref)
    print(f"quantiles vs the float64 bisection: max |dq| {d.max():.3e}; vs the float32 restatement {np.abs(got - co['q32'][:6]).max():.3e}")
    assert (d <= 1e-3 + 1e-4 * np.abs(ref)).all()  # the reference's own acceptance (:573)
    rc2, q2, _ = raw_quantiles(theta)
    torch.cuda.synchronize()
    assert rc2 == 0 and torch.equal(q.view(torch.int32), q2.view(torch.int32))  # bit-equal from run to run
    # a target that is not bracketed returns the bound it lies beyond; a bracketed one beside it is searched as before
    rc, qb, _ = raw_quantiles(theta, np.array([-1e30, 0.0, 1e30], np.float32))
    rc50, q50, _ = raw_quantiles(theta, radius=50.0)
    torch.cuda.synchronize()
    assert rc == 0 and (qb[:, 0] == -U.SEARCH_RADIUS).all() and (qb[:, 2] == U.SEARCH_RADIUS).all() and torch.equal(qb[:, 1], q[:, 1])
    inside = torch.from_numpy(np.abs(co["q32"]) < 49.0).to(DEV)
    assert rc50 == 0 and (q50[~inside].abs() == 50.0).all() and ((q50 - q)[inside].abs() <= 1e-3).all() and not inside[5, 0] and inside[1].all()
    # one channel alone: the same bits as among the others
    rc1, q1, _ = raw_quantiles(theta[4:5].contiguous())
    torch.cuda.synchronize()
    assert rc1 == 0 and torch.equal(q1[0], q[4])


def test_quantiles_of_nan_parameters_are_nan_and_the_call_returns(corpus):
    theta = corpus["theta"].clone()
    theta[3, 20] = float("nan")
    theta[2, 57] = float("inf")  # an infinite bias of the last layer: every chain value +inf, no NaN
    rc, q, g = raw_quantiles(theta)
    rc0, q0, _ = raw_quantiles(corpus["theta"])
    torch.cuda.synchronize()
    assert rc == 0 and rc0 == 0 and g.intact()
    assert torch.isnan(q[3]).all() and (q[2] == -U.SEARCH_RADIUS).all()  # +inf lies above every target: the lower bound
    keep = [0, 1, 4, 5, 6]
    assert torch.equal(q[keep], q0[keep])
    # the tables of such a model are refused, the channel named, nothing written
    rc, pmf, cdf, failed, intact = raw_tables(theta, dv(corpus["start"]), dv(corpus["length"]), corpus["stride"])
    torch.cuda.synchronize()
    assert rc == 1 and failed == 3 and intact and (cdf == HOST_FILL).all() and bool(torch.isnan(pmf).all())  # (channel 2's row is valid: the tail holds all)
    assert b"channel 3" in _lib.lib().fgmm_last_error()


def test_table_refusals_name_the_channel_and_write_nothing(corpus):
    theta = corpus["theta"][:2].contiguous()
    start = dv(np.array([-30.0, -40000.0], np.float32))
    for length, stride, want in (([61, 65536], 65537, 1), ([61, 0], 70, 1), ([70, 5], 70, 0), ([-3, 5], 70, 0)):
        rc, pmf, cdf, failed, intact = raw_tables(theta, start, dv(np.array(length, np.int32)), stride)
        torch.cuda.synchronize()
        assert rc == 1 and failed == want and intact and (cdf == HOST_FILL).all() and bool(torch.isnan(pmf).all()), (length, stride)
    assert b"channel 0" in _lib.lib().fgmm_last_error()
    rc, pmf, cdf, failed, intact = raw_tables(theta, start, dv(np.array([61, 9], np.int32)), 70)
    assert rc == 0 and failed == -1 and intact and not bool(torch.isnan(pmf).any())


# ---- d. the caller's stream ---------------------------------------------------------------------------------------------------------------
def test_both_calls_with_a_pending_producer(corpus, streams, delay):  # noqa: F811
    s1, s2, third = streams
    theta, start, length = corpus["theta"], dv(corpus["start"]), dv(corpus["length"])
    true = [theta, start, length]
    decoy = [theta.flip(0).contiguous(), start + 3.0, torch.clamp(length - 1, min=1)]
    _, q_w, _ = raw_quantiles(theta)
    torch.cuda.synchronize()
    assert not torch.equal(raw_tables(*decoy, corpus["stride"])[1], corpus["pmf"])
    with pending(s1, delay, true, decoy) as t:
        rc, pmf, cdf, failed, intact = raw_tables(t[0], t[1], t[2], corpus["stride"])
        pmf_3, = snapshot(third, [pmf])  # the call has returned: its outputs are complete
    assert rc == 0 and intact and torch.equal(pmf_3, corpus["pmf"]) and np.array_equal(cdf, corpus["cdf"])
    with pending(s2, delay, true, decoy) as t:
        rc, q, g = raw_quantiles(t[0])  # stream-ordered: queued behind the producer, complete once the stream is
    assert rc == 0 and g.intact() and torch.equal(q.view(torch.int32), q_w.view(torch.int32))


# ---- e. the module ------------------------------------------------------------------------------------------------------------------------
def corpus_module(corpus, quantiles=True):
    eb = EntropyBottleneck(U.C7)
    with torch.no_grad():
        for n in R.NAMES:
            getattr(eb, n).copy_(torch.from_numpy(corpus["co"]["params"][n]))
        if quantiles:
            eb.quantiles.copy_(torch.from_numpy(corpus["co"]["q32"]).reshape(U.C7, 1, 3))
    return eb.to(DEV)


class RefKeys(torch.nn.Module):
    """a stand-in that has the reference's state-dict keys and nothing else, the tables at the sizes given"""

    def __init__(self, like):
        super().__init__()
        for k, v in like.items():
            owner = self
            *path, leaf = k.split(".")
            for name in path:
                if not hasattr(owner, name):
                    owner.add_module(name, torch.nn.Module())
                owner = getattr(owner, name)
            owner.register_buffer(leaf, torch.zeros_like(v))


def test_module_update(corpus):
    eb = corpus_module(corpus)
    with pytest.raises(RuntimeError, match="update"):
        eb.coder()
    with warnings.catch_warnings(record=True) as caught:  # channel 6's single mass leaves half of it to the tail: said, not hidden
        warnings.simplefilter("always")
        assert eb.update() is True
    caught = [str(w.message) for w in caught if "tail_mass" in str(w.message)]
    assert len(caught) == 1 and "channel 6" in caught[0] and "update_quantiles" in caught[0]
    assert eb.update() is False
    with pytest.warns(UserWarning):
        assert eb.update(force=True) is True
    assert eb._quantized_cdf.shape == (U.C7, max(U.LENGTHS) + 2) and eb._cdf_length.shape == eb._offset.shape == (U.C7,)
    assert all(t.dtype == torch.int32 and t.device == eb.quantiles.device for t in (eb._quantized_cdf, eb._cdf_length, eb._offset))
    assert np.array_equal(eb._offset.cpu().numpy(), corpus["offset"]) and np.array_equal(eb._cdf_length.cpu().numpy(), corpus["length"] + 2)
    assert np.array_equal(eb._quantized_cdf.cpu().numpy(), corpus["cdf"])  # the raw call's, bit for bit
    assert eb.update_report["pmf_length"] == list(U.LENGTHS)
    assert np.array_equal(np.float32(eb.update_report["tail_mass"]), corpus["pmf"].cpu().numpy()[np.arange(U.C7), corpus["length"]])
    sd = eb.state_dict()
    fresh = EntropyBottleneck(U.C7)
    fresh.load_state_dict(sd, strict=True)
    assert all(torch.equal(fresh.state_dict()[k].cpu(), v.cpu()) for k, v in sd.items())
    g12 = np.load(os.path.join(ROOT, "tests", "golden", "g12_eb_update.npz"))
    assert {k[3:] for k in g12.files if k.startswith("sd.")} == set(sd)  # the reference's keys, no more and no fewer
    RefKeys(sd).load_state_dict(sd, strict=True)


def test_module_reproduces_the_references_tables_on_untrained_quantiles(g11):
    eb = EntropyBottleneck(R.C)
    sd = {k[3:]: torch.from_numpy(v) for k, v in g11.items() if k.startswith("sd.")}
    eb.load_state_dict(sd, strict=True)
    eb = eb.to(DEV)
    assert eb.update() is False  # the checkpoint's tables are there
    with pytest.warns(UserWarning, match="tail_mass"):
        assert eb.update(force=True) is True
    assert np.array_equal(eb._offset.cpu().numpy(), g11["sd._offset"]) and np.array_equal(eb._cdf_length.cpu().numpy(), g11["sd._cdf_length"])
    assert abs(eb.update_report["tail_mass"][5] - 0.755) < 1e-3
    p, q = {n: g11["p." + n] for n in R.NAMES}, g11["sd.quantiles"][:, 0, :]
    _, start, length = U.support(q)
    u64, ref32 = U.update(p, q, torch.float64), U.masses(p, start, length, torch.float32, device=DEV)
    tau = 2 * max(U.e_rel(ref32[0], u64["pmf"]), U.e_rel(ref32[1], u64["tail"])) + 2.0 ** -23
    got = eb._quantized_cdf.cpu().numpy()
    assert got.shape == g11["sd._quantized_cdf"].shape
    for c in range(R.C):
        ok, idx, flipped = U.table_admissible(got[c], U.entries(u64["pmf"], u64["tail"], u64["length"], c), tau)
        print(f"channel {c}: tau {tau:.3e}, {len(idx)} undecided, rounded the other way {flipped}; equal to the reference's: {np.array_equal(got[c], g11['sd._quantized_cdf'][c])}")
        assert ok and (flipped or np.array_equal(got[c], g11["sd._quantized_cdf"][c]))


def draw_z(corpus, seed, B=2, h=5, w=7):
    """values around each channel's median at the width of its support, and a few far beyond it: those take the bypass path"""
    rng = np.random.default_rng(seed)
    q = corpus["co"]["q32"]
    z = q[None, :, 1, None, None] + rng.standard_normal((B, U.C7, h, w)) * ((q[:, 2] - q[:, 0]) / 6.0 + 1.0)[None, :, None, None]
    z[0, :, 0, 0], z[1, :, 1, 2], z[1, :, 4, 6] = q[:, 2] + 40.0, q[:, 0] - 700.0, q[:, 1] + 3.0e4
    return dv(z.astype(np.float32))


def test_module_codes_on_its_tables(corpus):
    eb = corpus_module(corpus)
    with pytest.warns(UserWarning):
        eb.update()
    z = draw_z(corpus, 5)
    strings = eb.compress(z)
    med = eb.quantiles.detach()[:, 0, 1].reshape(1, -1, 1, 1)
    sym = torch.round(z - med)
    beyond = (sym < eb._offset.reshape(1, -1, 1, 1)) | (sym > (eb._offset + eb._cdf_length - 3).reshape(1, -1, 1, 1))
    assert int(beyond.sum()) >= 3 * U.C7 and int((~beyond).sum()) > beyond.numel() // 2
    assert torch.equal(eb.decompress(strings, z.shape[-2:]), sym + med)
    u32 = U.update(corpus["co"]["params"], corpus["co"]["q32"], torch.float32)
    ref = EntropyBottleneckCoder(torch.from_numpy(u32["cdf"]), torch.from_numpy(u32["cdf_length"]), torch.from_numpy(u32["offset"]),
                                 torch.from_numpy(corpus["co"]["q32"][:, 1].copy()))
    equal = np.array_equal(u32["cdf"], corpus["cdf"])
    print("the module's tables equal the float32 restatement's:", equal, " bytes per item:", [len(s) for s in strings])
    assert equal and ref.compress(z) == strings
    # changed parameters, a second update: compress codes on the new tables
    first = eb.coder()
    with torch.no_grad():
        eb._bias4 += 0.75
        eb._matrix0 -= 0.25
    assert eb.update(force=True, update_quantiles=True) is True and eb.coder() is not first
    assert max(eb.update_report["tail_mass"]) < 10 * eb.tail_mass and not torch.equal(eb.quantiles.detach().cpu()[:, 0], torch.from_numpy(corpus["co"]["q32"]))
    again = eb.compress(z)
    own = EntropyBottleneckCoder(eb._quantized_cdf, eb._cdf_length, eb._offset, eb.quantiles.detach()[:, 0, 1])
    assert again == own.compress(z) and again != strings
    med = eb.quantiles.detach()[:, 0, 1].reshape(1, -1, 1, 1)
    assert torch.equal(eb.decompress(again, z.shape[-2:]), torch.round(z - med) + med)


def test_module_refusals_leave_it_as_it_was(corpus):
    eb = corpus_module(corpus)
    with pytest.warns(UserWarning):
        eb.update()
    before = {k: v.clone() for k, v in eb.state_dict().items()}
    report = eb.update_report
    with torch.no_grad():
        eb.quantiles[2, 0, 0], eb.quantiles[2, 0, 2] = -40000.0, 40000.0
    before["quantiles"] = eb.quantiles.detach().clone()
    with pytest.raises(ValueError, match="channel 2"):
        eb.update(force=True)
    with torch.no_grad():
        eb._matrix2[4] = float("nan")
    before["_matrix2"] = eb._matrix2.detach().clone()
    with pytest.raises(ValueError, match="channel 4"):
        eb.update(force=True, update_quantiles=True)  # its quantiles are NaN: nothing is written, the searched quantiles neither
    with torch.no_grad():
        eb.quantiles[2, 0, 0], eb.quantiles[2, 0, 2] = -10.0, 10.0
    before["quantiles"] = eb.quantiles.detach().clone()
    with pytest.raises(ValueError, match="channel 4"):
        eb.update(force=True)  # a NaN mass, found by the call
    after = eb.state_dict()
    assert all(torch.equal(after[k].view(torch.int32) if after[k].is_floating_point() else after[k], before[k].view(torch.int32) if before[k].is_floating_point() else before[k])
               for k in before)
    assert eb.update_report is report
    cpu = EntropyBottleneck(2)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        cpu.update()


# ---- f. end to end ------------------------------------------------------------------------------------------------------------------------
def test_hyperprior_codec_end_to_end_on_fresh_modules():
    """train -> update() -> compress(): a HyperpriorLatentCodec over a fresh EntropyBottleneck, its tables built here"""
    from flashgmm_amd.latent_codecs import CheckerboardLatentCodec, GaussianMixtureConditionalLatentCodec, HyperLatentCodec, HyperpriorLatentCodec

    c, cz, c_side, h, w = 4, 3, 5, 16, 16
    Ctx, Par = T.exact_modules()
    Ha, Hs = T.exact_hyper_modules()
    torch.manual_seed(9)
    ycodec = CheckerboardLatentCodec(latent_codec={"y": GaussianMixtureConditionalLatentCodec(K=4)},
                                     context_prediction=Ctx(c, 2 * c), entropy_parameters=Par(2 * c + c_side, c))
    codec = HyperpriorLatentCodec(latent_codec={"y": ycodec, "hyper": HyperLatentCodec(entropy_bottleneck=EntropyBottleneck(cz), h_a=Ha(c, cz), h_s=Hs(cz, c_side))}).to(DEV)
    eb = codec["hyper"].entropy_bottleneck
    y, _ = T.exact_codec_inputs(41, c, c_side, h, w)
    y = dv(y)
    with pytest.raises(RuntimeError, match="update"):
        codec.compress(y)
    assert float(flashgmm_amd.aux_loss(codec).detach()) > 0
    assert flashgmm_amd.update_entropy_models(codec, update_quantiles=True) is True and flashgmm_amd.update_entropy_models(codec) is False
    assert max(eb.update_report["tail_mass"]) < eb.tail_mass and float(flashgmm_amd.aux_loss(codec).detach()) < 3 * cz * 1e-2
    enc = codec.compress(y)
    dec = codec.decompress(enc["strings"], enc["shape"])
    assert torch.equal(dec["y_hat"], enc["y_hat"])
    z = codec["hyper"].h_a(y)
    _, bits = eb.rate_bits(z, training=False)
    print(f"z strings: {[len(s) for s in enc['strings'][-1]]} bytes; rate_bits(z, training=False) / 8: {(bits / 8).tolist()} bytes; "
          f"pmf_length {eb.update_report['pmf_length']}")
