"""CPU: the launch forms of the calls that price latents (estimate, RDOQ, curve, budget; weighted; channel skip) as tests/enc_ref.py
restates them, and the conditions under which the sweep of tests/test_gpu_enc_forms.py over ``enc_ref.ODD_CORPUS`` shows something -
computed on the reference side alone (tests/rdoq_ref.py, rdcurve_ref.py, rdo_weights_ref.py, rdo_skip_ref.py), for every mode, clamped
and not, at lambda = 0.5.  They are conditions on the corpus (its seeds and scales were chosen to meet them), not measurements."""
import pytest
import torch

from flashgmm_amd import _lib
from tests import enc_ref as F
from tests import rdcurve_ref as V
from tests import rdo_skip_ref as S
from tests import rdo_weights_ref as W
from tests import rdoq_ref as Q
from tests import synth as T

LIN, TILED = F.LIN, F.TILED


def item(M, hw, planes_off=0, y_off=0, out_off=0, stride_c=None, stride_k=None):
    """a dense item (or one of the given strides); the offsets are bytes past a 16-byte boundary"""
    stride_c = hw if stride_c is None else stride_c
    return F.form_item(hw, stride_c, M * stride_c if stride_k is None else stride_k, (planes_off,) * 3, y_off, out_off)


#        items, two-byte planes, pos_w pointers (None: not weighted), the form
TABLE = [([item(12, 8 * 13)], False, None, (4, TILED)),  # hw = 104 = 4 * 26: NOT the 1-wide path - 26 lanes of one wave
         ([item(12, 8 * 13)], True, None, (4, TILED)),
         ([item(12, 7 * 9)], False, None, (1, TILED)),  # hw = 63
         ([item(8, 16)], False, None, (4, TILED)),
         ([item(32, 128)], False, None, (4, TILED)),  # 128 is no multiple of 256
         ([item(32, 128, y_off=4)], False, None, (1, LIN)),  # ... but of 64
         ([item(16, 256)], False, None, (4, LIN)),
         ([item(16, 256)], True, None, (4, LIN)),
         ([item(16, 256, y_off=4)], False, None, (1, LIN)),
         ([item(16, 256, out_off=4)], False, None, (1, LIN)),  # the output alone
         ([item(16, 256, planes_off=8)], False, None, (1, LIN)),  # float32 planes want 16 bytes ...
         ([item(16, 256, planes_off=8)], True, None, (4, LIN)),  # ... two-byte planes 8
         ([item(16, 256, planes_off=2)], True, None, (1, LIN)),
         ([item(3, 16, stride_c=18)], False, None, (1, TILED)),  # by the channel stride alone
         ([item(3, 16, stride_c=20)], False, None, (4, TILED)),
         ([item(3, 16, stride_k=50)], False, None, (1, TILED)),  # by the component stride alone
         ([item(4, 16)], False, [0], (4, TILED)),  # weighted, without position factors
         ([item(4, 16)], False, [4], (1, TILED)),  # by pos_w alone
         ([item(4, 256)], False, [16], (4, LIN)),
         ([item(4, 256), item(2, 512)], False, None, (4, LIN)),  # every hw a multiple of 256
         ([item(4, 256), item(2, 64)], False, None, (4, TILED)),
         ([item(4, 256), item(2, 64, y_off=4)], False, None, (1, LIN)),  # one misaligned item takes the batch to 1-wide: 64 | 256
         ([item(4, 256), item(2, 63)], False, None, (1, TILED)),
         ([item(4, 256), item(0, 21)], False, None, (1, TILED)),  # an item without channels still decides
         ([item(4, 256), item(2, 256)], False, [0, 4], (1, LIN)),
         ([item(1, 1)], False, None, (1, TILED)), ([item(1, 3)], True, None, (1, TILED)), ([item(1, 4)], True, None, (4, TILED)),
         ([item(5, 260)], False, None, (4, TILED)), ([item(2, 257)], False, None, (1, TILED)), ([item(2, 64)], False, None, (4, TILED))]


def test_the_launch_form_on_hand_written_cases():
    for items, two_byte, pos_w, want in TABLE:
        assert F.latent_launch_form(items, two_byte, pos_w) == want, (items, two_byte, pos_w)
    assert F.latent_launch_form([item(12, 104)], False) == (4, TILED)  # the shape the family's modules called "odd: the 1-wide path"


def test_the_items_are_read_off_the_tensors():
    """``items_of`` on host tensors laid out as the GPU module lays out its device tensors: the form is the planned one"""
    M, h, w = 3, 4, 4
    y = torch.zeros(1, M, h, w)
    dense = [torch.zeros(1, 4 * M, h, w) for _ in range(3)]
    want = F.latent_launch_form([item(M, 16, planes_off=dense[0].data_ptr() % 16, y_off=y.data_ptr() % 16)], False)
    assert F.form_of_one(y, *dense, pos_w=False) == want
    assert F.items_of([y], *([t] for t in dense))[0]["stride_c"] == 16
    buf = torch.zeros(4 * M * 18 + 8)
    strided = [torch.as_strided(buf, (1, 4 * M, h, w), (4 * M * 18, 18, w, 1)) for _ in range(3)]
    it = F.items_of([y], *([t] for t in strided))[0]
    assert (it["hw"], it["stride_c"], it["stride_k"]) == (16, 18, 54) and F.form_of_one(y, *strided, pos_w=False) == (1, TILED)
    off = torch.zeros(M * 16 + 1)[1:].view(1, M, h, w)  # one float into its storage
    assert F.items_of([off], *([t] for t in dense))[0]["y"] == off.data_ptr() == off.untyped_storage().data_ptr() + 4
    two =[t.to(torch.bfloat16) for t in dense]
    assert F.items_of([y], *([t] for t in two))[0]["planes"][0] == two[0].data_ptr()
    st = F.items_of(torch.zeros(2, M, h, w), *(torch.zeros(2, 4 * M, h, w) for _ in range(3)))
    assert len(st) == 2 and st[1]["y"] - st[0]["y"] == 4 * M * 16 and st[1]["planes"][0] - st[0]["planes"][0] == 4 * 4 * M * 16
    with pytest.raises(AssertionError):
        F.items_of([y], *([t.transpose(2, 3)] for t in dense))


def test_the_corpus_reaches_the_four_forms_with_every_plane_type():
    hws = lambda ids: sorted(F.ODD_CORPUS[i][1] * F.ODD_CORPUS[i][2] for i in ids)  # noqa: E731
    for pt in F.PLANE_TYPES:
        for weighted in (False, True):
            forms = {F.planned_form(i, pt, weighted) for i in range(len(F.ODD_CORPUS))}
            assert forms == {(1, TILED), (4, TILED), (1, LIN), (4, LIN)}, (pt, weighted)
        assert hws(F.entries_of_form((1, TILED), pt)) == [1, 3, 16, 21, 63, 65, 255, 257], pt  # (16: by stride alone)
        assert hws(F.entries_of_form((4, TILED), pt)) == [4, 16, 252, 260], pt  # (16: the pos_w entry, without weights)
        assert hws(F.entries_of_form((1, LIN), pt)) == [64, 128] and hws(F.entries_of_form((4, LIN), pt)) == [256], pt
        assert hws(F.entries_of_form((1, TILED), pt, weighted=True)) == [1, 3, 16, 16, 21, 63, 65, 255, 257], pt  # by pos_w alone
    assert all(1 <= M <= 5 for M, _, _, _ in F.ODD_CORPUS) and max(M * h * w for M, h, w, _ in F.ODD_CORPUS) == 5 * 260
    assert set(F.DEAD) == {"first", "last", "all_but_one", "none"} and len(F.DEAD) == len(F.ODD_CORPUS)
    assert sum(M == 1 for M, _, _, _ in F.ODD_CORPUS) == 2


def test_the_derived_cases_reach_every_instantiation():
    rate, rdoq, curve = F.instantiations()
    tf = (True, False)
    want_rate = {(mode, vec, clamp, pt, linear) for mode in F.MODES for vec in (1, 4) for clamp in tf for pt in F.PLANE_TYPES for linear in tf}
    want = {r + (weighted, skip) for r in want_rate for weighted in tf for skip in tf}
    assert len(want_rate) == 72 and len(want) == 288
    assert rate == want_rate and rdoq == want and curve == want


# ---- the conditions that keep the GPU sweep from passing vacuously ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def swept(oracle):
    """{(mode, clamp, plane type): per entry (case as the reference is fed it, its candidates priced, the plain RDOQ reference at LAM)}"""
    L = _lib.lib()
    out = {}
    for mode in F.MODES:
        for clamp in (True, False):
            for pt in F.PLANE_TYPES:
                rows = []
                for i in range(len(F.ODD_CORPUS)):
                    case = F.widened_case(i, clamp, pt)
                    rows.append((case, V.price(oracle, L, mode, *case, clamp=clamp), Q.rdoq(oracle, L, mode, *case, F.LAM, clamp=clamp)))
                out[mode, clamp, pt] = rows
    return out


def test_the_planted_layouts_are_what_is_coded(swept):
    for key, rows in swept.items():
        for i, (case, p, r) in enumerate(rows):
            M, h, w, _ = F.ODD_CORPUS[i]
            dead = F.dead_channels(i)
            zb = [int(c not in dead) for c in range(M)]
            assert T.to_coder_inputs(*case, clamp=key[1])[5].tolist() == zb, (key, i)
            assert case[0][0, dead].all() if dead else True  # (dead channels hold latents, none of them zero)
            assert r["n_coded"] == (M - len(dead)) * h * w > 0, (key, i)


def test_moves_exist_and_go_both_ways_and_meet_the_bypass(swept):
    for key, rows in swept.items():
        moved = sum(r["n_changed"] for _, _, r in rows)
        coded = sum(r["n_coded"] for _, _, r in rows)
        print(key, "moved", moved, "of", coded, "away", sum(r["n_away"] for _, _, r in rows), "bypass candidates", sum(r["n_bypass_cand"] for _, _, r in rows))
        assert moved * 20 >= coded, (key, moved, coded)
        for i, (_, _, r) in enumerate(rows):
            if F.ODD_CORPUS[i][1] * F.ODD_CORPUS[i][2] >= 21:
                assert r["n_changed"] >= 1, (key, i)
        assert sum(r["n_away"] for _, _, r in rows) >= 1, key
        assert sum(r["n_bypass_cand"] for _, _, r in rows) >= 1, key
        # the weighted decisions differ from the plain ones somewhere: the factors are not idle
        diff = 0
        for i, (case, p, r) in enumerate(rows):
            cw, pw = F.factors(i)
            diff += int((W.choose(p, F.LAM, W.weights_of(*case, cw, pw, clamp=key[1]))[0] != W.choose(p, F.LAM, W.weights_of(*case, clamp=key[1]))[0]).sum())
        assert diff >= 1, key


def test_channels_are_skipped_and_kept_in_both_widths(swept):
    for key, rows in swept.items():
        for weighted in (False, True):
            skipped = kept = skipped_1wide = kept_1wide = inelig = 0
            for i, (case, p, _) in enumerate(rows):
                M, h, w, _ = F.ODD_CORPUS[i]
                cw, pw = F.factors(i) if weighted else (None, None)
                ch = S.channels(p, F.LAM, W.weights_of(*case, cw, pw, clamp=key[1]), h * w)
                skipped += int(ch["skip"].sum())
                kept += int((~ch["skip"] & ~ch["inelig"]).sum())
                inelig += int(ch["inelig"].sum())
                if F.planned_form(i, key[2], weighted)[0] == 1:  # the 1-wide zero store runs, and is held back
                    skipped_1wide += int(ch["skip"].sum())
                    kept_1wide += int((~ch["skip"] & ~ch["inelig"]).sum())
            print(key, "weighted" if weighted else "plain", "skipped", skipped, "eligible kept", kept, "1-wide", skipped_1wide, kept_1wide, "ineligible", inelig)
            assert skipped >= 1 and kept >= 1 and skipped_1wide >= 1 and kept_1wide >= 1 and inelig >= 1, (key, weighted)
