"""Shared by tests/test_census_cpu.py and tests/test_gpu_census.py: the corpus that holds the kernels AROUND the coder to the oracle -
``quant_stats_kernel`` and ``chan_compact_kernel`` in front of every encode and pricing call, ``yhat_scatter_kernel``,
``yhat_scatter_round_kernel`` and ``yhat_zero_dead_kernel`` behind every decode call (flashgmm_amd/csrc/fgmm_kernels.hip).

The corpus is built by PLACING values, never by drawing them: a census that is wrong at one position of one wave does not show on a
random latent.  Nothing is stored: ``expect`` is ``tests/synth.to_coder_inputs`` (the reference's entropy_models.py:834-845 restated) and
the bytes are ``oracle.encode_gmm``'s.  numpy only.

What the census kernel decides inside itself is restated here: ``stats_path`` (the float4 path needs hw a multiple of 4 and y and the
y_q output 16-byte aligned; a channel's row then is too) and ``lane_of`` (which trip, wave, lane and float4 component reads a position).

Families:
  sizes       hw in SIZES, M = 3: the item's maximum on the first position of channel 0, its minimum - which sets abs_max - on the last
              position of channel 2, channel 1 dead.  PLACEMENTS: aligned; y one element in; the y_q output one element in; two items
              that are views 0 and 2 of one [3, M, 1, hw] storage.
  sweep       hw in SWEEP_HW, one KIND of value on one position of ``sweep_positions(hw)`` of a channel that is otherwise 0.25 (dead,
              abs_max 1).  ``sweep_item``: one channel per position and a last one without a value - the zero bitmap and y_q see every
              position.  abs_max is one number per ITEM, so there a lost extreme hides behind the other channels': ``sweep_solo`` is the
              same channel as an item of its own (M = 1), a batch of them is one launch.  A NaN alone cannot show in abs_max either
              (NaN gives 1, and so does 0.25): the solo kind "nan_among" puts -3.3 and +5.5 on two other positions, in other waves
              where the size has them - a NaN lost from the minimum gives 4, from the maximum 6, kept in both 1.  +inf shows in the
              zero bitmap, y_q and the bytes only (|inf|.int() is INT32_MIN, as for NaN).
  rounding    ROUNDING: one group of values per item, with the outcome the group forces (dead or live, abs_max); y_q bit patterns.
  compaction  M in COMPACT_M, hw 3 or 5, the live channels by name (``live_sets``): both sides of 63 | 64, 255 | 256, 511 | 512, a
              chunk of 256 without a live channel in front of a live one, a wave without one."""
from __future__ import annotations

import functools

import numpy as np

from tests import synth as T

BLOCK, WAVE = 256, 64
MODE = "polya"
STRIDE = 256  # the smallest checkpoint stride the library takes
DECODE_MAX = 40000  # items beyond this abs_max are compressed only
SEED = 9100
PLANE_KINDS = ("float32", "float16")


# ---- the kernel's own decisions ---------------------------------------------------------------------------------------------------------
def stats_path(hw, y_addr, yq_addr=0):
    """quant_stats_kernel's choice, from hw and the byte addresses it is handed (yq_addr 0: no y_q output)"""
    return "float4" if hw % 4 == 0 and y_addr % 16 == 0 and yq_addr % 16 == 0 else "scalar"


def lane_of(path, p):
    """-> (trip, wave, lane, float4 component) of the thread that reads position p of a channel"""
    if path == "float4":
        t = (p % (4 * BLOCK)) // 4
        return p // (4 * BLOCK), t // WAVE, t % WAVE, p % 4
    t = p % BLOCK
    return p // BLOCK, t // WAVE, t % WAVE, 0


class Item:
    """one latent with its planes: y [1, M, h, w], (sigma, mu, pi) [1, 4M, h, w] float32 (sigma before the clamp)"""

    def __init__(self, name, y, planes, **info):
        self.name, self.y, self.planes, self.info = name, np.ascontiguousarray(y, dtype=np.float32), planes, info
        _, self.M, self.h, self.w = self.y.shape
        self.hw = self.h * self.w

    def device_planes(self, kind="float32"):
        """-> (what the device is handed, the float32 values it stands for)"""
        if kind == "float32":
            return self.planes, self.planes
        p = T.to_float16_planes(*self.planes)
        return p, tuple(a.astype(np.float32) for a in p)

    def expect(self, kind="float32", clamp=True):
        """-> dict: sym, rows (sigma, mu, pi as the coder gets them), am, zb, yq, nz (the compact channel list)"""
        sym, s, m, w, am, zb, yq = T.to_coder_inputs(self.y, *self.device_planes(kind)[1], clamp=clamp)
        return dict(sym=sym, rows=(s, m, w), am=am, zb=zb, yq=yq, nz=np.nonzero(zb)[0])

    def decodable(self, kind="float32", clamp=True):
        """can a decoder be handed the item's own abs_max?  Not beyond DECODE_MAX (a decoder's tables span 2 * (abs_max + 1) + 2 edges
        per latent), and not "nan_among": a NaN makes abs_max 1 whatever else the latent holds (entropy_models.py:834-837), and the
        window of that half-width misses the -3 and the 5 the encoder coded - in the reference as here"""
        return self.expect(kind, clamp)["am"] <= DECODE_MAX and not self.info.get("window_misses")

    def decoded(self, kind="float32", clamp=True):
        """what decompress returns: the symbols as floats in their channels, +0.0 everywhere else"""
        e = self.expect(kind, clamp)
        out = np.zeros((self.M, self.hw), np.float32)
        out[e["nz"]] = e["sym"].astype(np.float32).reshape(len(e["nz"]), self.hw)
        return out.reshape(self.y.shape)


@functools.lru_cache(maxsize=None)
def _planes(M, h, w):
    return tuple(T.make_latent(SEED + 7 * M + h * w, M, h, w, clamp=False)[1:])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """float bit patterns, -0.0 distinct from +0.0; a NaN equals any NaN (the host makes the negative default NaN where the GPU makes
    the positive one, and no test here computes with one)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- sizes ------------------------------------------------------------------------------------------------------------------------------
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1020, 1024, 1028, 2052)
PLACEMENTS = ("aligned", "y_off", "yq_off", "batch_view")
SIZE_M = 3
SIZE_ABS_MAX = 21  # from -20.7 on the last position of the last channel


@functools.lru_cache(maxsize=None)
def size_item(hw, second=False):
    """``second``: the other item of the batch_view placement (other values, the same structure)"""
    M = SIZE_M
    y = np.clip(T.make_latent(SEED + hw + (500 if second else 0), M, 1, hw)[0], -15, 15).astype(np.float32)
    y[0, 1, 0] = np.where(np.arange(hw) % 2 == 0, 0.25, -0.3).astype(np.float32)  # dead, and not zero
    y[0, 0, 0, 0] = 17.6
    y[0, 2, 0, hw - 1] = -20.7
    return Item(f"size hw={hw}{' second' if second else ''}", y, _planes(M, 1, hw))


def planned_addresses(hw, placement):
    """-> [(y address, y_q address)] of the items of the call, every allocation at address 0"""
    if placement == "batch_view":
        return [(0, 0), (2 * SIZE_M * hw * 4, 0)]
    return [(4 if placement == "y_off" else 0, 4 if placement == "yq_off" else 0)]


def planned_paths(hw, placement):
    return [stats_path(hw, ya, qa) for ya, qa in planned_addresses(hw, placement)]


# ---- position sweep ---------------------------------------------------------------------------------------------------------------------
SWEEP_HW = (65, 257, 1028, 2052)
KINDS = {"nonzero": 7.0, "neg": -9.4, "nan": float("nan"), "inf": float("inf")}
SOLO_KINDS = ("nonzero", "neg", "nan_among")
SOLO_ABS_MAX = {"nonzero": 8, "neg": 10, "nan_among": 1}
AMONG = (-3.3, 5.5)  # the companions of the NaN in "nan_among": without the NaN abs_max is 6, with it lost from the minimum alone 4
BACKGROUND = 0.25


def sweep_positions(hw):
    path = stats_path(hw, 0)
    per = 4 if path == "float4" else 1  # positions per lane and trip
    pos = [0, 3, 4, 63, 64, 252, 255, 256, per * BLOCK - 1, hw - 4, hw - 1]
    pos += [per * 2 * WAVE, per * 3 * WAVE - 1, per * 3 * WAVE]  # (wave 2's first and last position of the first trip, wave 3's first)
    if hw > 4 * BLOCK:  # a second trip of the float4 path
        pos += [1023, 1024, 1027]
    if hw > 8 * BLOCK:  # a third
        pos += [2047, 2048]
    return sorted({p for p in pos if 0 <= p < hw})


@functools.lru_cache(maxsize=None)
def sweep_item(hw, kind):
    pos = sweep_positions(hw)
    M = len(pos) + 1
    y = np.full((1, M, 1, hw), BACKGROUND, np.float32)
    for j, p in enumerate(pos):
        y[0, j, 0, p] = KINDS[kind]
    return Item(f"sweep hw={hw} {kind}", y, _planes(M, 1, hw), positions=pos)


def among_positions(hw, p):
    """the positions of "nan_among"'s two companions: read by another wave than p where the size has one, never p"""
    path, pos = stats_path(hw, 0), sweep_positions(hw)
    far = [q for q in pos if q != p and lane_of(path, q)[1] != lane_of(path, p)[1]] + [q for q in pos if q != p]
    q1 = far[0]
    q2 = [q for q in reversed(far) if q != q1][0]
    return q1, q2


@functools.lru_cache(maxsize=None)
def sweep_solo(hw, kind, p):
    y = np.full((1, 1, 1, hw), BACKGROUND, np.float32)
    if kind == "nan_among":
        q1, q2 = among_positions(hw, p)
        y[0, 0, 0, q1], y[0, 0, 0, q2] = AMONG
        y[0, 0, 0, p] = np.nan
    else:
        y[0, 0, 0, p] = KINDS[kind]
    return Item(f"solo hw={hw} {kind} at {p}", y, _planes(1, 1, hw), position=p, window_misses=kind == "nan_among")


def sweep_solos(hw, kind):
    return [sweep_solo(hw, kind, p) for p in sweep_positions(hw)]


# ---- rounding and sign ------------------------------------------------------------------------------------------------------------------
F = np.float32
ROUNDING = [  # (name, the values a channel holds, live, abs_max)
    ("half_and_below", [0.5, -0.5, -0.3, float(np.nextafter(F(0.5), F(0))), 1e-45, -1e-45, 1.1754942e-38], False, 1),  # -0.0 where y < 0
    ("above_half", [float(np.nextafter(F(0.5), F(1)))], True, 1),   # 0.50000006 -> 1; int(0.50000006) + 1 = 1
    ("ties", [1.5, 2.5, -1.5, -2.5], True, 3),                      # half to even: 2, 2, -2, -2
    ("large", [8388607.5, 16777216.0], True, 16777217),              # the last half below 2^23 (-> 8388608), the end of exact integers
]
ROUND_HW = (12, 13)  # the float4 path and the scalar one


@functools.lru_cache(maxsize=None)
def rounding_item(name, hw):
    vals = np.array(next(r[1] for r in ROUNDING if r[0] == name), np.float32)
    row = vals[np.arange(hw) % len(vals)]
    y = np.stack([row, row[::-1]]).reshape(1, 2, 1, hw)
    return Item(f"rounding {name} hw={hw}", y, _planes(2, 1, hw))


# ---- compaction -------------------------------------------------------------------------------------------------------------------------
COMPACT_M = (1, 64, 65, 256, 257, 513)


def compact_hw(M):
    return 5 if M % 2 else 3


def live_sets(M):
    """-> {name: the live channels}, each set once (M = 1: "first" is "all")"""
    sets = {"all": list(range(M)), "none": [], "first": [0], "last": [M - 1], "alternate": list(range(0, M, 2))}
    for a, b in ((63, 64), (255, 256), (511, 512)):
        if b < M:
            sets[f"{a}_{b}"] = [a, b]
    if M > 256:
        sets["256"] = [256]                                       # chunk 0 without a live channel (M = 257: "last", chunk 1 entirely live)
    if M >= 512:
        sets["chunk1_only"] = list(range(256, 512))               # chunk 0 entirely dead, chunk 1 entirely live (channel 512 dead)
    if M >= 128:
        sets["wave1_dead"] = [c for c in range(M) if not 64 <= c < 128]
    out, seen = {}, set()
    for name, s in sets.items():
        if tuple(s) not in seen:
            seen.add(tuple(s))
            out[name] = s
    return out


COMPACT_CASES = [(M, name) for M in COMPACT_M for name in live_sets(M)]


@functools.lru_cache(maxsize=None)
def compact_item(M, name, outlier=False):
    """live channel c holds the integers ((5 c + 3 p) mod 9) - 4 plus a quarter (three different ones: something is coded), a dead
    one 0.25 and -0.3 in turn.  ``outlier``: one latent of the middle live channel is 70000.4 - a symbol beyond int16"""
    hw, live = compact_hw(M), live_sets(M)[name]
    p = np.arange(hw)
    y = np.tile(np.where(p % 2 == 0, 0.25, -0.3).astype(np.float32), (M, 1))
    for c in live:
        y[c] = ((5 * c + 3 * p) % 9 - 4 + 0.25).astype(np.float32)
    if outlier:
        y[live[len(live) // 2], hw // 2] = 70000.4
    return Item(f"compact M={M} {name}{' outlier' if outlier else ''}", y.reshape(1, M, 1, hw), _planes(M, 1, hw), live=live)


OUTLIER_CASE = (65, "alternate")
# one call of the sequence form: M = 513 next to M = 1, an all-dead item between two live ones
BATCH_CASES = [(513, "alternate"), (1, "all"), (64, "none"), (257, "last"), (1, "none"), (513, "chunk1_only"), (65, "63_64")]


GENERIC_ABS_MAX = 7  # the smallest abs_max whose window (2 * (abs_max + 1) + 2 = 18 edges) the single-pass kernel cannot take at tab_cap_e = 256


def decode_items():
    """what the decode-side tests decode: every compaction item, the rounding items a decoder can be handed, a few sizes and sweeps"""
    items = [compact_item(M, name) for M, name in COMPACT_CASES]
    items += [rounding_item(name, hw) for name, *_ in ROUNDING for hw in ROUND_HW]
    items += [size_item(hw) for hw in (1, 5, 63, 257, 1028)]
    items += [sweep_item(hw, k) for hw in (65, 1028) for k in ("nonzero", "neg")]
    return [it for it in items if it.decodable()]


def first_wrong_channel(oracle, got_bytes, e, hw):
    """what a failure names: the first channel of the expected compact list whose symbols, decoded from the bytes the GPU path made,
    differ from the expected ones (None: the bytes do not decode, or decode to the same symbols)"""
    try:
        got = oracle.decode_gmm(MODE, got_bytes, *e["rows"], e["am"] + 1)
    except Exception:  # noqa: BLE001 - whatever the oracle makes of foreign bytes
        return None
    bad = np.nonzero(got != e["sym"])[0]
    return None if len(bad) == 0 else int(e["nz"][bad[0] // hw])
