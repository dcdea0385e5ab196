"""CPU: section 3k of include/flashgmm_amd.h - the entropy bottleneck's update() - without a device.  The header, the exports and the
binding; the restatement of tests/eb_update_ref.py (the arithmetic the GPU tests hold the kernels to) against the reference's own class:
its tables on untrained quantiles (tests/golden/g11_entropy_bottleneck.npz) and after ``update(force=True, update_quantiles=True)``
(tests/golden/g12_eb_update.npz, written by tests/golden/make_golden_eb_update.py); what the corpus claims to contain; refusals that need
no device; ``update_entropy_models`` / ``aux_loss`` over a stand-in tree; the coder's cache key.

THE DECIDED-ENTRY RULE.  The masses enter a table in one place, the quantiser's first step round(m * 2^16).  With tau = 2 * E_ref + 2^-23,
E_ref the error of torch's float32 mirrored form against float64 (relative, floor 2^-17), an entry is DECIDED when m64 * 2^16 is
farther from a half-integer than tau * max(m64 * 2^16, 1); two correct float32 evaluations may round an undecided entry either way.
Measured on the corpus: E_ref 5.2e-5 (the chain amplifies the rounding of its sums by the logit), so tau 1.0e-4 and 5 to 17 undecided
entries per channel of 27 to 1022 - not the two at the most that a tau near 2^-23 would leave.  The reference's own float32 run on
g12 goes the other way in one of them (channel 5, entry 555: m * 2^16 = 322.4992).  Without the masses a table is therefore compared as
``table_admissible`` does: the float64 table with at most two undecided entries rounded the other way; with them, ``counts_admissible``."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import flashgmm_amd
from flashgmm_amd import EntropyBottleneck, _lib
from tests import eb_ref as R
from tests import eb_update_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g11():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g11_entropy_bottleneck.npz")))


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g12_eb_update.npz")))


@pytest.fixture(scope="module")
def restated():
    """the restatement on the corpus' own quantiles, float32 and float64: computed once, left unchanged"""
    co = U.corpus()
    return {dt: U.update(co["params"], co["q32"], dt) for dt in (torch.float32, torch.float64)}


def test_header_exports_and_binding():
    header = open(os.path.join(ROOT, "include", "flashgmm_amd.h")).read()
    assert re.search(r"^#define FGMM_HAS_EB_UPDATE 1\b", header, re.M) and " 3k. " in header
    assert re.search(r"^#define FGMM_ABI_VERSION 6\b", header, re.M) and _lib.lib().fgmm_abi_version() == 6  # added without a bump
    assert int(re.search(r"^#define FGMM_EB_SEARCH_CAP (\d+)\b", header, re.M).group(1)) == _lib.FGMM_EB_SEARCH_CAP
    want = {"fgmm_eb_quantiles": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_float), C.c_float, C.c_void_p],
            "fgmm_eb_tables": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int32)]}
    for name, args in want.items():
        proto = re.search(r"^int " + name + r"\(([^;]*)\);", header, re.M | re.S).group(1)
        assert len(proto.split(",")) == len(args)  # parameter for parameter, as the header declares them
        assert hasattr(_lib.lib(), name) and _lib.SIGNATURES[name] == (C.c_int, args)
    # both Python boundaries reach the calls the way they reach section 3j's: through the library's C ABI (the compiled module and its
    # stand-in carry the batched coder calls only), so the one binding serves either
    assert _lib.boundary() is not None and not any("eb_" in n for n in dir(_lib.boundary()) if not n.startswith("_"))
    for name in ("update_entropy_models", "aux_loss"):
        assert callable(getattr(flashgmm_amd, name)) and name in flashgmm_amd.entropy_models.__all__
    assert callable(EntropyBottleneck.update) and callable(EntropyBottleneck._update_quantiles)
    assert "NaN" in header[header.index(" 3k. "):header.index("int fgmm_eb_quantiles")]  # the value of a search that cannot be made is stated


def test_restated_tables_equal_the_references_on_untrained_quantiles(g11):
    """quantiles (-10, med, 10): 22 masses per channel and tails up to 0.755; float32 and float64, mirrored and written form, each
    reproduce the reference's 6 x 24 table bit for bit (all lengths are equal: the tail is the reference's)"""
    p, q = {n: g11["p." + n] for n in R.NAMES}, g11["sd.quantiles"][:, 0, :]
    assert g11["sd._quantized_cdf"].shape == (6, 24)
    for dtype in (torch.float32, torch.float64):
        for mirrored in (True, False):
            u = U.update(p, q, dtype, mirrored=mirrored)
            assert np.array_equal(u["offset"], g11["sd._offset"]) and u["offset"].dtype == np.int32
            assert np.array_equal(u["cdf_length"], g11["sd._cdf_length"])
            assert np.array_equal(u["cdf"], g11["sd._quantized_cdf"]), (dtype, mirrored)
    print("tails", u["tail"].tolist())
    assert abs(float(u["tail"][5]) - 0.755) < 1e-3  # what update() warns about


def test_restated_bisection_lies_within_the_references_acceptance(g12):
    co = U.corpus()
    for name, q in (("float32", co["q32"][:6]), ("float64", co["q64"][:6])):
        for ref_name, ref in (("the reference's float32 run", g12["sd.quantiles"][:, 0, :]), ("its float64 search", g12["q64"])):
            d = np.abs(q.astype(np.float64) - ref)
            print(f"bisection {name} vs {ref_name}: max |dq| {d.max():.3e}")
            assert (d <= 1e-3 + 1e-4 * np.abs(ref)).all()  # the reference's own atol / rtol (:573)
    d = np.abs(co["q32"][:6].astype(np.float64) - co["q64"][:6])
    print(f"float32 vs float64 restatement: max |dq| {d.max():.3e}")
    assert (d <= 1e-3 + 1e-4 * np.abs(co["q64"][:6])).all()
    assert np.array_equal(co["q32"][6], np.full(3, co["q32"][1, 1])) and np.isfinite(co["q32"]).all()


def test_bisection_edges():
    """a target that is not bracketed collapses onto the bound it lies beyond; NaN parameters give NaN; each search is its channel's own"""
    _, p, _, _, _ = R.corpus()
    q = U.bisect(p, torch.float32, tgt=np.array([-1e30, 0.0, 1e30], np.float32)).numpy()
    assert (q[:, 0] == -U.SEARCH_RADIUS).all() and (q[:, 2] == U.SEARCH_RADIUS).all() and np.array_equal(q[:, 1], U.corpus()["q32"][:6, 1])
    bad = {n: a.copy() for n, a in p.items()}
    bad["_bias2"][3, 1, 0] = np.nan
    qb = U.bisect(bad, torch.float32).numpy()
    assert np.isnan(qb[3]).all() and np.array_equal(np.delete(qb, 3, 0), np.delete(U.corpus()["q32"][:6], 3, 0))
    one = U.bisect({n: a[4:5] for n, a in p.items()}, torch.float32).numpy()
    assert np.array_equal(one[0], U.corpus()["q32"][4])


def test_restated_tables_on_the_references_bisected_quantiles(g12):
    p, q = {n: g12["p." + n] for n in R.NAMES}, g12["sd.quantiles"][:, 0, :]
    u32, u64 = U.update(p, q, torch.float32), U.update(p, q, torch.float64)
    assert np.array_equal(u64["offset"], g12["sd._offset"]) and np.array_equal(u64["cdf_length"], g12["sd._cdf_length"])
    assert g12["sd._quantized_cdf"].shape == u64["cdf"].shape == (6, 1024) and tuple(u64["length"]) == U.LENGTHS[:6]
    e_ref = U.e_rel(u32["pmf"], u64["pmf"])
    tau = 2 * e_ref + 2.0 ** -23
    print(f"E_ref {e_ref:.3e}  tau {tau:.3e}")
    for c in range(6):
        prob64 = U.entries(u64["pmf"], u64["tail"], u64["length"], c)
        ok, idx, flipped = U.table_admissible(g12["sd._quantized_cdf"][c], prob64, tau)
        m = prob64 * 65536.0
        print(f"channel {c}: {len(idx)} undecided of {len(prob64)}, the reference's table rounds {flipped} the other way "
              f"(m * 2^16 {[round(float(m[i]), 4) for i in flipped or []]})")
        assert ok, (c, idx)
        assert not g12["sd._quantized_cdf"][c, len(prob64) + 1:].any()  # zero-padded (:206-214)
        # the tail as the reference takes it - at the longest channel's last sample - gives the same tables here: either is below 1e-9
        ref_tail = U.masses(p, u64["start"], u64["length"], torch.float64, tail_at_longest=True)[1]
        assert ref_tail[c] <= u64["tail"][c] < U.TAIL_MASS


def test_float32_and_float64_restatements_agree_on_the_corpus(restated):
    u32, u64 = restated[torch.float32], restated[torch.float64]
    assert tuple(u32["length"]) == U.LENGTHS and all((n + 1) % 64 for n in U.LENGTHS) and max(U.LENGTHS) > 3 * 256 and min(U.LENGTHS) == 1
    assert (u32["tail"][:6] < U.TAIL_MASS).all() and (u64["tail"][:6] < U.TAIL_MASS).all() and u32["tail"][6] > 0.1
    print("tails", u64["tail"].tolist())
    for c in range(U.C7):
        assert np.array_equal(u32["cdf"][c], u64["cdf"][c]), c
    tau = 2 * U.e_rel(u32["pmf"], u64["pmf"]) + 2.0 ** -23
    for c in range(U.C7):
        ok, idx, off = U.counts_admissible(U.entries(u32["pmf"], u32["tail"], u32["length"], c), U.entries(u64["pmf"], u64["tail"], u64["length"], c), tau)
        print(f"channel {c}: {len(idx)} undecided, float32 rounds {off} the other way")
        assert ok
    m = np.concatenate([U.entries(u64["pmf"], u64["tail"], u64["length"], c) for c in range(U.C7)]) * 65536.0
    print(f"smallest relative margin to a half-integer: {(np.abs(m - np.floor(m) - 0.5) / np.maximum(m, 1.0)).min():.2e}")


def test_the_decided_entry_rule_has_teeth(restated):
    u64 = restated[torch.float64]
    prob64 = U.entries(u64["pmf"], u64["tail"], u64["length"], 0)
    row = u64["cdf"][0]
    assert U.table_admissible(row, prob64, 1e-4)[0]
    wrong = row.copy()
    wrong[100:200] += 1  # one count moved between two decided entries
    assert not U.table_admissible(wrong, prob64, 1e-4)[0]
    decided = [i for i in range(len(prob64)) if i not in U.undecided(prob64, 1e-4) and prob64[i] * 65536 > 10][0]
    moved = prob64.astype(np.float32).copy()
    moved[decided] += np.float32(1.0 / 65536)
    assert not U.counts_admissible(moved, prob64, 1e-4)[0] and U.counts_admissible(prob64.astype(np.float32), prob64, 1e-4)[0]


def test_refusals_without_a_device():
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p, fake = buf.ctypes.data, buf.ctypes.data  # (a refused call reads neither)
    tg = (C.c_float * 3)(-1.0, 0.0, 1.0)
    assert L.fgmm_eb_quantiles(None, None, p, 1, tg, 1e5, p) == 1 and L.fgmm_eb_quantiles(fake, None, None, 1, tg, 1e5, p) == 1
    assert L.fgmm_eb_quantiles(fake, None, p, 1, None, 1e5, p) == 1 and L.fgmm_eb_quantiles(fake, None, p, 1, tg, 1e5, None) == 1
    assert L.fgmm_eb_quantiles(fake, None, p, 0, tg, 1e5, p) == 1
    for radius in (0.0, -1.0, float("inf"), float("nan")):
        assert L.fgmm_eb_quantiles(fake, None, p, 1, tg, radius, p) == 1
    assert L.fgmm_eb_quantiles(fake, None, p, 1, (C.c_float * 3)(-1.0, float("nan"), 1.0), 1e5, p) == 1
    assert b"NaN" in L.fgmm_last_error()
    failed = C.c_int32(-7)
    for args in ((None, None, p, p, p, 1, 4, None, p), (fake, None, None, p, p, 1, 4, None, p), (fake, None, p, None, p, 1, 4, None, p),
                 (fake, None, p, p, None, 1, 4, None, p), (fake, None, p, p, p, 1, 4, None, None), (fake, None, p, p, p, 0, 4, None, p),
                 (fake, None, p, p, p, 1, 1, None, p), (fake, None, p, p, p, 1 << 16, 1 << 16, None, p)):
        assert L.fgmm_eb_tables(*args, C.byref(failed)) == 1
    assert failed.value == -7 and not buf.any()
    eb = EntropyBottleneck(3)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        eb.update()
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        eb._update_quantiles()
    assert eb._offset.numel() == 0 and eb.update_report is None
    eb._offset = torch.zeros(3, dtype=torch.int32)
    assert eb.update() is False  # the tables are there: nothing to do, no device needed


class _Recorder(EntropyBottleneck):
    def __init__(self, channels, answer):
        super().__init__(channels)
        self.answer, self.calls = answer, []

    def update(self, force=False, update_quantiles=False):
        self.calls.append((force, update_quantiles))
        return self.answer


def test_update_entropy_models_and_aux_loss_over_a_tree():
    torch.manual_seed(3)
    a, b, c = _Recorder(2, False), _Recorder(3, True), _Recorder(1, False)
    tree = torch.nn.Sequential(torch.nn.Conv2d(2, 2, 1), a, torch.nn.ModuleDict({"inner": torch.nn.Sequential(b), "other": torch.nn.ReLU()}))
    assert flashgmm_amd.update_entropy_models(tree) is True and a.calls == b.calls == [(False, False)]
    assert flashgmm_amd.update_entropy_models(tree, force=True, update_quantiles=True) is True and a.calls[-1] == b.calls[-1] == (True, True)
    assert flashgmm_amd.update_entropy_models(c, force=True) is False and c.calls == [(True, False)]  # the root itself counts
    assert flashgmm_amd.update_entropy_models(torch.nn.ReLU()) is False
    loss = flashgmm_amd.aux_loss(tree)
    assert torch.equal(loss, a.loss() + b.loss()) and loss.requires_grad and float(loss.detach()) > 0
    loss.backward()
    assert a.quantiles.grad is not None and a._matrix0.grad is None  # the quantiles alone (stop_gradient on the rest)
    assert flashgmm_amd.aux_loss(torch.nn.ReLU()) == 0


def test_coder_sees_freshly_assigned_tables(g11):
    """a freshly assigned tensor has ``_version`` 0 like the one it replaces: the cache key looks at the storage too"""
    eb = EntropyBottleneck(R.C)
    eb.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g11.items() if k.startswith("sd.")}, strict=True)
    keep = []  # (the replaced tensors are held, so that a new one cannot take the address of an old one)
    coders = []
    for a, b in ((7, 11), (13, 17)):
        table = eb._quantized_cdf.numpy().copy()
        table[:, 1:3] = [a, b]
        keep.append(eb._quantized_cdf)
        eb._quantized_cdf = torch.from_numpy(table)
        assert eb._quantized_cdf._version == 0
        coders.append(eb.coder())
        assert eb.coder() is coders[-1] and np.array_equal(coders[-1]._tables.mat[:, 1:3], np.tile(np.array([a, b], np.int32), (R.C, 1)))
    assert coders[0] is not coders[1]
