"""CPU: the corpus of tests/census_ref.py has what tests/test_gpu_census.py relies on - every listed position is reached by every
kind of value, in every wave, in the last float4 component and in a partial trip; each rounding group forces the outcome its table row
states; every compaction set has the live channels it claims, on both sides of 64, 256 and 512; the census kernel's two paths are reached
as the placements plan them; and every item round-trips through the oracle's coder."""
import numpy as np
import pytest

from tests import census_ref as R


def test_sweep_reaches_every_position_with_every_kind():
    for hw in R.SWEEP_HW:
        path, pos = R.stats_path(hw, 0), R.sweep_positions(hw)
        assert path == ("float4" if hw in (1028, 2052) else "scalar")
        assert {0, 3, 4, 63, 64, hw - 4, hw - 1} <= set(pos) and (hw < 257 or {252, 255, 256} <= set(pos))
        where = [R.lane_of(path, p) for p in pos]
        trips = 1 + (hw - 1) // (1024 if path == "float4" else 256)
        assert {t for t, *_ in where} == set(range(trips))  # every trip, the partial last one with it
        assert R.lane_of(path, hw - 1)[0] == trips - 1
        if hw >= 257:
            assert {w for _, w, _, _ in where} == {0, 1, 2, 3}
            assert (0, 0, 63) in {x[:3] for x in where} and (0, 3, 0) in {x[:3] for x in where}  # wave 0's last lane, wave 3's first
            assert (0, 3, 63) in {x[:3] for x in where}  # the last position of wave 3's first trip
        if path == "float4":
            assert {1023, 1024, 1027} <= set(pos) and {c for *_, c in where} == {0, 3}
        for kind, v in R.KINDS.items():
            it = R.sweep_item(hw, kind)
            assert it.M == len(pos) + 1 and it.info["positions"] == pos
            for j, p in enumerate(pos):
                off = np.nonzero(R.bits(it.y[0, j, 0]) != R.bits(np.float32(R.BACKGROUND)))[0]
                assert off.tolist() == [p] and R.same_bits(it.y[0, j, 0, p], np.float32(v)), (hw, kind, p)
            assert np.all(it.y[0, -1] == R.BACKGROUND)
            e = it.expect()
            assert e["zb"].tolist() == [1] * len(pos) + [0]  # the value alone makes its channel live
            assert e["am"] == {"nonzero": 8, "neg": 10, "nan": 1, "inf": 1}[kind]


def test_solo_items_show_their_value_in_abs_max():
    for hw in R.SWEEP_HW:
        path = R.stats_path(hw, 0)
        for kind in R.SOLO_KINDS:
            items = R.sweep_solos(hw, kind)
            assert [it.info["position"] for it in items] == R.sweep_positions(hw)
            for it in items:
                e, p = it.expect(), it.info["position"]
                assert it.M == 1 and e["am"] == R.SOLO_ABS_MAX[kind] and e["zb"].tolist() == [1]
                y = it.y.copy()
                if kind != "nan_among":  # without the value: dead, abs_max 1
                    y[0, 0, 0, p] = R.BACKGROUND
                    lost = R.Item("lost", y, it.planes).expect()
                    assert (lost["am"], lost["zb"].tolist()) == (1, [0])
                    continue
                q1, q2 = R.among_positions(hw, p)
                assert len({p, q1, q2}) == 3 and (y[0, 0, 0, q1], y[0, 0, 0, q2]) == tuple(np.float32(R.AMONG)) and np.isnan(y[0, 0, 0, p])
                assert R.lane_of(path, q1)[1] != R.lane_of(path, p)[1]  # the minimum's companion: folded by another wave
                y[0, 0, 0, p] = R.BACKGROUND
                assert R.Item("lost", y, it.planes).expect()["am"] == 6  # a NaN lost from both folds; from the minimum alone: 3 + 1


ROUND_BITS = {  # y_q of the first channel's first len(values) positions, as bit patterns
    "half_and_below": [0x00000000, 0x80000000, 0x80000000, 0x00000000, 0x00000000, 0x80000000, 0x00000000],
    "above_half": [0x3F800000],
    "ties": [0x40000000, 0x40000000, 0xC0000000, 0xC0000000],
    "large": [0x4B000000, 0x4B800000],
}


@pytest.mark.parametrize("hw", R.ROUND_HW)
def test_rounding_groups_force_their_outcome(hw):
    assert {R.stats_path(h, 0) for h in R.ROUND_HW} == {"float4", "scalar"}
    for name, vals, live, am in R.ROUNDING:
        it = R.rounding_item(name, hw)
        e = it.expect()
        assert set(R.bits(it.y).reshape(-1).tolist()) == set(R.bits(np.array(vals, np.float32)).tolist()), name
        assert e["zb"].tolist() == [int(live)] * 2 and e["am"] == am, (name, e["zb"], e["am"])
        assert R.bits(e["yq"][0, 0, 0, :len(vals)]).tolist() == ROUND_BITS[name][:hw], name
    assert float(np.float32(0.49999997)) == R.ROUNDING[0][1][3] and float(np.float32(0.50000006)) == R.ROUNDING[1][1][0]


def test_compaction_sets_are_what_they_claim():
    assert len(R.COMPACT_CASES) == len(set(R.COMPACT_CASES))
    for M in R.COMPACT_M:
        sets = R.live_sets(M)
        assert {"all", "none"} <= set(sets) and len({tuple(s) for s in sets.values()}) == len(sets)
        for name, live in sets.items():
            it = R.compact_item(M, name)
            e = it.expect()
            assert (it.M, it.hw) == (M, R.compact_hw(M)) and e["nz"].tolist() == live and e["am"] in ((4, 5) if live else (1,)), (M, name)
            assert len(e["sym"]) == len(live) * it.hw and np.all(it.y != 0)  # a dead channel is not a zero channel
    count = {(M, name): len(s) for M in R.COMPACT_M for name, s in R.live_sets(M).items()}
    assert count[513, "all"] == 513 and count[513, "alternate"] == 257 and count[513, "chunk1_only"] == 256 and count[513, "wave1_dead"] == 449
    assert count[513, "256"] == 1 and count[257, "last"] == 1 and (257, "256") not in count and count[64, "last"] == 1 and count[1, "all"] == 1 and (1, "first") not in count
    # both sides of 64, 256 and 512: a live channel just below and just above each boundary, and a live one above a dead stretch
    assert R.live_sets(65)["63_64"] == [63, 64] and R.live_sets(257)["255_256"] == [255, 256] and R.live_sets(513)["511_512"] == [511, 512]
    for b, M in ((64, 65), (256, 257), (512, 513)):
        assert R.live_sets(M)["last"] == [b] and b - 1 in R.live_sets(b)["last"]
    assert min(R.live_sets(513)["chunk1_only"]) == 256 and max(R.live_sets(513)["chunk1_only"]) == 511
    w1 = R.live_sets(513)["wave1_dead"]
    assert 63 in w1 and 128 in w1 and not set(range(64, 128)) & set(w1)
    for M, name in R.BATCH_CASES + [R.OUTLIER_CASE]:
        assert name in R.live_sets(M)
    Ms = [M for M, _ in R.BATCH_CASES]
    assert Ms[:2] == [513, 1] and any(R.BATCH_CASES[i][1] == "none" and 0 < i < len(Ms) - 1 for i in range(len(Ms)))


def test_both_paths_are_reached_as_the_placements_plan():
    """aligned and batch_view reach the float4 path at every hw that is a multiple of 4 and the scalar path at every other; y_off and
    yq_off are scalar at EVERY size - at the multiples of 4 by the address alone, which is what they are for"""
    for placement in R.PLACEMENTS:
        by_path = {"float4": set(), "scalar": set()}
        for hw in R.SIZES:
            for path in R.planned_paths(hw, placement):
                by_path[path].add(hw)
        mult4 = {hw for hw in R.SIZES if hw % 4 == 0}
        assert mult4 == {4, 64, 256, 1020, 1024, 1028, 2052}
        if placement in ("aligned", "batch_view"):
            assert by_path["float4"] == mult4 and by_path["scalar"] == set(R.SIZES) - mult4, placement
        else:
            assert not by_path["float4"] and by_path["scalar"] == set(R.SIZES), placement
    # one trip, one trip and one lane, two trips and one lane of the float4 path
    assert [R.lane_of("float4", hw - 1)[:3] for hw in (1024, 1028, 2052)] == [(0, 3, 63), (1, 0, 0), (2, 0, 0)]
    for hw in R.SIZES:
        it = R.size_item(hw)
        e = it.expect()
        assert e["am"] == R.SIZE_ABS_MAX and e["zb"].tolist() == [1, 0, 1]
        assert float(it.y.max()) == float(np.float32(17.6)) and float(it.y.min()) == float(np.float32(-20.7))
        assert it.y[0, 2, 0, hw - 1] == it.y.min() and np.abs(np.delete(it.y.reshape(-1), [0, 3 * hw - 1])).max() <= 15


def _all_items():
    for hw in R.SIZES:
        yield R.size_item(hw)
        yield R.size_item(hw, True)
    for hw in R.SWEEP_HW:
        for kind in R.KINDS:
            yield R.sweep_item(hw, kind)
        for kind in R.SOLO_KINDS:
            yield from R.sweep_solos(hw, kind)
    for name, *_ in R.ROUNDING:
        for hw in R.ROUND_HW:
            yield R.rounding_item(name, hw)
    for M, name in R.COMPACT_CASES:
        yield R.compact_item(M, name)
    yield R.compact_item(*R.OUTLIER_CASE, outlier=True)


def test_every_item_round_trips_through_the_oracle(oracle):
    n = 0
    for it in _all_items():
        for kind in R.PLANE_KINDS if it.name.startswith(("sweep", "compact")) else ("float32",):
            e = it.expect(kind)
            data = oracle.encode_gmm(R.MODE, e["sym"], *e["rows"])
            if len(e["sym"]) == 0:
                assert len(data) == 8, it.name  # the stream of an empty item: the flushed state
            if not it.decodable(kind):
                assert it.name.startswith("rounding large") or "outlier" in it.name or "nan_among" in it.name, it.name
                continue
            assert np.array_equal(oracle.decode_gmm(R.MODE, data, *e["rows"], e["am"] + 1), e["sym"]), (it.name, kind)
            n += 1
    assert n > 200
    # the outlier is coded by the bypass escape: a half-width without it decodes the stream as well (the rounds then meet a symbol
    # beyond int16)
    it, clean = R.compact_item(*R.OUTLIER_CASE, outlier=True), R.compact_item(*R.OUTLIER_CASE)
    e = it.expect()
    assert e["am"] == 70001 and clean.expect()["am"] == 5 and e["nz"].tolist() != list(range(len(e["nz"])))
    data = oracle.encode_gmm(R.MODE, e["sym"], *e["rows"])
    assert np.array_equal(oracle.decode_gmm(R.MODE, data, *e["rows"], 5 + 1), e["sym"]) and int(e["sym"].max()) == 70000


def test_decode_items_decode_under_a_wider_window_too(oracle):
    """the generic table kernels take an item only when its window has more than 16 edges: the GPU test hands the items with a
    smaller abs_max GENERIC_ABS_MAX instead - the oracle decodes the same symbols under it"""
    items = R.decode_items()
    assert len(items) >= 50 and sum(len(it.expect()["sym"]) > R.STRIDE for it in items) >= 10 and sum(it.expect()["am"] < R.GENERIC_ABS_MAX for it in items) >= 30
    assert 256 // (2 * (R.GENERIC_ABS_MAX + 1) + 2) < 16 <= 256 // (2 * R.GENERIC_ABS_MAX + 2)
    for it in items:
        e = it.expect()
        data = oracle.encode_gmm(R.MODE, e["sym"], *e["rows"])
        assert np.array_equal(oracle.decode_gmm(R.MODE, data, *e["rows"], max(e["am"], R.GENERIC_ABS_MAX) + 1), e["sym"]), it.name


def test_first_wrong_channel_names_the_channel(oracle):
    """the failure message of the GPU test: bytes coded from a compact list with one wrong entry name the channel that entry stands for"""
    it = R.compact_item(65, "63_64")
    e, hw = it.expect(), it.hw
    assert R.first_wrong_channel(oracle, oracle.encode_gmm(R.MODE, e["sym"], *e["rows"]), e, hw) is None
    wrong = [63, 62]  # the list a census would give that took channel 62 for channel 64
    sym = np.round(it.y[0, wrong]).reshape(-1).astype(np.int32)
    rows = [p.reshape(4, it.M, hw)[:, wrong].reshape(4, -1).T for p in it.planes]
    rows[0] = np.clip(rows[0], np.float32(0.11), np.float32(256))
    assert R.first_wrong_channel(oracle, oracle.encode_gmm(R.MODE, sym, *rows), e, hw) == 64
    assert R.first_wrong_channel(oracle, b"\x00" * 3, e, hw) is None
